// kai_session_update.hpp — kai_session_update / kai_session_update_rows: the arguments' check, the update in its phases, the wrapper that closes the session when a failure comes after the first write.
#pragma once
#include "kai_session_open.hpp"
namespace {
// ---- kai_session_update: a pod / node delta applied to the open session's snapshot (include/kai_core.h).  Phases: (1) the arguments, on the host; (2) the delta staged
// and sent in one copy, k_delta_gather reads the snapshot's side of every changed pod (no write); (3) the open's refusals against S', on the host; (4) the counters the
// open derives by walking the pods and nodes, adjusted old -> new, and the class table ranked again (host, proportional to the delta); (5) k_apply_delta scatters into
// the baselines, the class labels are re-derived if the table changed, and the session math is re-derived on the device as kai_session_reset does.
// kai_session_update_rows adds the rows (the clock, queue rows, job start times): checked with the delta in (1), staged behind it in the same buffer and sent by the same
// copy in (2), HostPrep::shares and the clock set in (4), k_apply_rows beside k_apply_delta in (5) — one re-derivation for both parts.
// One call's state, shared by the phases: the host and device sides of the staging buffer (DeltaLayout, kai_delta.hpp), the gather's output, the delta's nodes in engine order.
struct SessionUpdate {
    kai_core* core; const kai_session_delta* dl; const kai_session_rows* rw;
    KaiCtx& c; HostPrep& prep; SharedPods& sp;
    const int N, P, R, NP, NN, NQ, NJ; const DeltaLayout L;
    unsigned char *pin = nullptr, *dv = nullptr;  // the staging buffer: pinned, device
    int32_t *h32 = nullptr, *hp = nullptr, *hs = nullptr, *hn = nullptr, *hg = nullptr, *hnode = nullptr; uint32_t* hflags = nullptr; double* h64 = nullptr;  // the delta as sent: pod, status, node, group | node, flags | [R][NN] allocatable
    const int32_t *old_st = nullptr, *old_nd = nullptr, *old_gr = nullptr, *cnt = nullptr; const uint32_t* pflag = nullptr;  // the gather's output: what the snapshot holds for every changed pod; the counters
    DeltaView v{}; RowsView rv{};
    // the delta's nodes in engine order (the node rows the host keeps are); engine nodes whose legacy-MIG bit may change (written with the delta's nodes); those of them outside the delta: appended as node entries of their own
    std::vector<int32_t> eng, touched, extra;
    int gpu_nodes_after = -1; bool cls_changed = false, remap_changed = false;
    SessionUpdate(kai_core* core_, const kai_session_delta* dl_, const kai_session_rows* rw_)
        : core(core_), dl(dl_), rw(rw_), c(core_->ctx), prep(core_->prep), sp(core_->sp), N(c.N), P(c.P), R(c.R), NP(dl_->n_pods), NN(dl_->n_nodes),
          NQ(rw_ ? rw_->n_queues : 0), NJ(rw_ ? rw_->n_jobs : 0), L(NP, NN, R, NQ, NJ, core_->legacy_on), eng((size_t)dl_->n_nodes) {}
    double node_row(int k, int r) const { const int e = eng[(size_t)k]; return dl->node_allocatable ? dl->node_allocatable[(size_t)r * NN + k] : prep.node_alloc[(size_t)r * N + e]; }
    int new_node(int i) const { return hn[i] >= 0 ? (int)prep.rank_of[(size_t)hn[i]] : -1; }

    // ---- (2) the delta staged and sent in one copy; k_delta_gather reads the snapshot's side of every changed pod (no write)
    int stage_and_gather() {
        KAI_TRY(reserve(core, core->dl_pin, L.total, L.total + L.total / 4));
        KAI_TRY(reserve(core, core->dl_dev, L.total, L.total + L.total / 4));
        pin = core->dl_pin.p; dv = core->dl_dev.p;
        if (!core->d_rank) {  // caller's node index -> engine index (name rank) on the device, once per session
            uint32_t* t = nullptr; int rc = dalloc(core, &t, (size_t)std::max(N, 1)); if (rc) return rc;
            if (N) HIP_TRY(core, hipMemcpyAsync(t, prep.rank_of.data(), (size_t)N * 4, hipMemcpyHostToDevice, core->stream));
            core->d_rank = t;
        }
        h32 = reinterpret_cast<int32_t*>(pin + L.o_i32); h64 = reinterpret_cast<double*>(pin + L.o_f64);
        hp = h32; hs = h32 + NP; hn = h32 + 2 * NP; hg = h32 + 3 * NP; hnode = h32 + 4 * NP; hflags = reinterpret_cast<uint32_t*>(h32 + 4 * NP + NN);
        for (int k = 0; k < NN; k++) eng[(size_t)k] = (int32_t)prep.rank_of[(size_t)dl->node[k]];
        for (int i = 0; i < NP; i++) {
            const int p = dl->pod[i]; hp[i] = p; hs[i] = dl->pod_status[i]; hn[i] = dl->pod_node[i];
            hg[i] = dl->pod_gpu_group ? (sp.shared.size() > (size_t)p && sp.shared[(size_t)p] ? dl->pod_gpu_group[i] : -1) : KD_KEEP;  // the open's rule: a group only on a shared-GPU request
        }
        for (int k = 0; k < NN; k++) {
            const int e = eng[(size_t)k]; hnode[k] = dl->node[k];
            hflags[k] = dl->node_flags ? ((dl->node_flags[k] & 0x0FFFFFFFu) | (prep.node_flags[(size_t)e] & 0xF0000000u)) : prep.node_flags[(size_t)e];  // the caller's bits masked as the open does, the library's own kept
            for (int r = 0; r < R; r++) h64[(size_t)r * NN + k] = node_row(k, r);
        }
        // the rows: an array the call leaves NULL takes no part (its slot in the buffer is sent as it is and never read)
        rv = RowsView{}; rv.n_queues = NQ; rv.n_jobs = NJ;
        {   unsigned char* dv0 = dv;
            int32_t* r32 = reinterpret_cast<int32_t*>(pin + L.o_r32); unsigned char* r64 = pin + L.o_r64;
            auto put = [&](size_t off, const void* src, size_t bytes) -> const void* { if (!src || !bytes) return nullptr; std::memcpy(r64 + off, src, bytes); return dv0 + L.o_r64 + off; };
            if (NQ) { std::memcpy(r32, rw->queue, (size_t)NQ * 4); rv.queue = reinterpret_cast<const int32_t*>(dv0 + L.o_r32);
                      if (rw->queue_priority) { std::memcpy(r32 + NQ, rw->queue_priority, (size_t)NQ * 4); rv.prio = reinterpret_cast<const int32_t*>(dv0 + L.o_r32) + NQ; } }
            if (NJ) { std::memcpy(r32 + 2 * NQ, rw->job, (size_t)NJ * 4); rv.job = reinterpret_cast<const int32_t*>(dv0 + L.o_r32) + 2 * NQ; }
            const size_t q3 = (size_t)3 * NQ * 8, q1 = (size_t)NQ * 8;
            rv.deserved = static_cast<const double*>(put(0, rw ? rw->queue_deserved : nullptr, q3)); rv.limit = static_cast<const double*>(put(q3, rw ? rw->queue_limit : nullptr, q3));
            rv.oqw = static_cast<const double*>(put(2 * q3, rw ? rw->queue_oqw : nullptr, q3)); rv.usage = static_cast<const double*>(put(3 * q3, rw ? rw->queue_usage : nullptr, q3));
            rv.preempt_mr = static_cast<const int64_t*>(put(4 * q3, rw ? rw->queue_preempt_min_runtime_ns : nullptr, q1));
            rv.reclaim_mr = static_cast<const int64_t*>(put(4 * q3 + q1, rw ? rw->queue_reclaim_min_runtime_ns : nullptr, q1));
            rv.last_start = static_cast<const int64_t*>(put(4 * q3 + 2 * q1, rw ? rw->job_last_start_ns : nullptr, (size_t)NJ * 8));
        }
        v = DeltaView{reinterpret_cast<const int32_t*>(dv), reinterpret_cast<const int32_t*>(dv) + NP, reinterpret_cast<const int32_t*>(dv) + 2 * NP, reinterpret_cast<const int32_t*>(dv) + 3 * NP,
                      reinterpret_cast<const int32_t*>(dv) + 4 * NP, reinterpret_cast<const uint32_t*>(dv) + 4 * NP + NN, reinterpret_cast<const double*>(dv + L.o_f64), NP, NN, R, N, core->d_rank};
        int32_t* d_out = reinterpret_cast<int32_t*>(dv + L.o_out); int32_t* d_cnt = reinterpret_cast<int32_t*>(dv + L.o_cnt);
        HIP_TRY(core, hipMemsetAsync(d_cnt, 0, 256, core->stream));
        HIP_TRY(core, hipMemcpyAsync(dv, pin, L.o_out, hipMemcpyHostToDevice, core->stream));
        if (NP) hipLaunchKernelGGL(k_delta_gather, dim3((NP + KD_TB - 1) / KD_TB), dim3(KD_TB), 0, core->stream, v, (const int32_t*)core->d_status0, (const int32_t*)core->d_node0,
                                   (const int32_t*)core->aux.group0, (const uint32_t*)KAI_VP(c.p_flags), d_out, d_cnt);
        HIP_TRY(core, hipGetLastError());
        HIP_TRY(core, hipMemcpyAsync(pin + L.o_out, d_out, L.o_cnt + 256 - L.o_out, hipMemcpyDeviceToHost, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        old_st = reinterpret_cast<const int32_t*>(pin + L.o_out); old_nd = old_st + NP; old_gr = old_st + 2 * NP;
        pflag = reinterpret_cast<const uint32_t*>(old_st + 3 * NP); cnt = reinterpret_cast<const int32_t*>(pin + L.o_cnt);
        return KAI_OK;
    }
    // ---- (3) the open's refusals on S' (the pods outside the delta passed them when S was opened)
    int refusals() {
        for (int i = 0; i < NP; i++) if ((pflag[i] & KAI_POD_CPU_FALLBACK) && hs[i] == KAI_POD_PENDING) return fail(core, KAI_ERR_UNSUPPORTED, "a pending pod is flagged KAI_POD_CPU_FALLBACK: leave its job to the host path");
        for (int i = 0; i < NP; i++) if ((pflag[i] & KAI_POD_GPU_UNMODELLED) && (hs[i] & KAI_POD_ACTIVE)) return fail(core, KAI_ERR_UNSUPPORTED, "an active pod holds GPU state the device does not model (gpu-memory / several fractional devices / MIG / DRA): its node's idle GPUs would be overstated");
        auto has_gpus = [&](auto row) { if (row(KAI_RES_GPU) > 0) return true; for (int r = KAI_RES_PODS + 1; r < R && r < KAI_MAX_RES; r++) if (sp.mig_g[r] > 0 && row(r) > 0) return true; return false; };
        if (core->gm_guard && dl->node_allocatable) {  // the open's rule on S': one GPU memory size among the nodes that have GPUs (SharedPods::build)
            int joined = 0, left = 0; int64_t v = -1; bool mixed = false;
            for (int k = 0; k < NN; k++) {
                const int e = eng[(size_t)k];
                const bool was = has_gpus([&](int r) { return prep.node_alloc[(size_t)r * N + e]; }), is = has_gpus([&](int r) { return node_row(k, r); });
                if (was && !is) left++;
                if (!was && is) { joined++; const int64_t m = core->h_gpu_mem[(size_t)e]; if (v < 0) v = m; else if (m != v) mixed = true; }
            }
            if (joined || left) {
                const bool stay = sp.n_gpu_nodes - left > 0;  // nodes of S that keep their GPUs: all of them carry sp.M
                if (mixed || (stay && joined && v != sp.M)) return fail(core, KAI_ERR_UNSUPPORTED, "shared GPUs with different node_gpu_memory values: leave the cycle to the host path");
                const int64_t m_new = stay ? sp.M : joined ? v : core->h_gpu_mem[(size_t)prep.rank_of[0]];
                if (m_new != sp.M) return fail(core, KAI_ERR_UNSUPPORTED, "kai_session_update: the cluster's GPU memory size would change (every GPU node replaced): open the new snapshot");
                gpu_nodes_after = sp.n_gpu_nodes + joined - left;
            }
        }
        return KAI_OK;
    }
    // ---- (4) the counters the open derives by walking the pods and nodes, adjusted old -> new; the class table ranked again; the rows' effect on the host's copies
    void host_bookkeeping() {
        if (gpu_nodes_after >= 0) core->sp.n_gpu_nodes = gpu_nodes_after;
        prep.n_relpipe += cnt[0];
        if (prep.keyed) for (int i = 0; i < NP; i++) {
            const int p = hp[i]; const int64_t d = (hs[i] == KAI_POD_PENDING ? 1 : 0) - (old_st[i] == KAI_POD_PENDING ? 1 : 0);
            if (!d) continue;
            if (sp.any && sp.shared[(size_t)p]) prep.n_pend_shared += d; else prep.cfreq[(size_t)prep.pod_key[(size_t)p]] += d;
        }
        if (core->legacy_on) for (int i = 0; i < NP; i++) {
            if (!(pflag[i] & KAI_POD_LEGACY_MIG)) continue;
            const int on = (old_st[i] & KAI_POD_ACTIVE) ? old_nd[i] : -1, nn = (hs[i] & KAI_POD_ACTIVE) ? new_node(i) : -1;
            if (on == nn) continue;
            if (on >= 0) { core->legacy_cnt[(size_t)on]--; touched.push_back(on); }
            if (nn >= 0) { core->legacy_cnt[(size_t)nn]++; touched.push_back(nn); }
        }
        // nodes: the class guard's and the exact-sum guard's counts, the host's rows (engine order), the legacy-MIG bit
        for (int k = 0; k < NN; k++) {
            const int e = eng[(size_t)k];
            if (dl->node_allocatable) {
                if (!prep.nsum_ready) prep.build_node_sums(R, N);  // (once per session: the exact-sum guard's node counts, from the rows before this delta)
                for (int t = 0; t < 2; t++) {
                    const int r = t == 0 ? KAI_RES_CPU : KAI_RES_GPU;
                    prep.nodes_bad[t] += (HostPrep::node_guard_fails(core->cfg, t, h64[(size_t)r * NN + k], prep.node_gpu_count[(size_t)e]) ? 1 : 0)
                                       - (HostPrep::node_guard_fails(core->cfg, t, prep.node_alloc[(size_t)r * N + e], prep.node_gpu_count[(size_t)e]) ? 1 : 0);
                }
                for (int r = 0; r < R; r++) { prep.nsum[r].add(prep.node_alloc[(size_t)r * N + e], -1); prep.nsum[r].add(h64[(size_t)r * NN + k], +1); prep.node_alloc[(size_t)r * N + e] = h64[(size_t)r * NN + k]; }
            }
            prep.node_flags[(size_t)e] = hflags[k];
        }
        std::sort(touched.begin(), touched.end()); touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
        for (int e : touched) {
            const uint32_t f = core->legacy_cnt[(size_t)e] > 0 ? (prep.node_flags[(size_t)e] | KAI_NODE_LEGACY_MIG_I) : (prep.node_flags[(size_t)e] & ~KAI_NODE_LEGACY_MIG_I);
            prep.node_flags[(size_t)e] = f;
            bool listed = false; for (int k = 0; k < NN && !listed; k++) if (eng[(size_t)k] == e) { hflags[k] = f; listed = true; }
            if (!listed) extra.push_back(e);
        }
        // shared GPUs: each node's active pods in UID order, and the groups the cycle may open (next_group0)
        if (core->shared) {
            for (int i = 0; i < NP; i++) {
                const int p = hp[i], on = (old_st[i] & KAI_POD_ACTIVE) ? old_nd[i] : -1, nn = (hs[i] & KAI_POD_ACTIVE) ? new_node(i) : -1;
                if (on == nn) continue;
                const std::pair<uint32_t, int32_t> key{core->np_uid[(size_t)p], p};
                if (on >= 0) { auto& L = core->np_lists[(size_t)on]; auto it = std::lower_bound(L.begin(), L.end(), key); if (it != L.end() && *it == key) L.erase(it); }
                if (nn >= 0) { auto& L = core->np_lists[(size_t)nn]; L.insert(std::lower_bound(L.begin(), L.end(), key), key); }
            }
            for (int i = 0; i < NP; i++) {
                if (hg[i] == KD_KEEP || hg[i] == old_gr[i]) continue;
                if (old_gr[i] >= KAI_NEW_GROUP) { auto it = core->new_groups.find(old_gr[i]); if (it != core->new_groups.end() && --it->second == 0) core->new_groups.erase(it); }
                if (hg[i] >= KAI_NEW_GROUP) core->new_groups[hg[i]]++;
            }
            core->next_group0 = core->new_groups.empty() ? KAI_NEW_GROUP : core->new_groups.rbegin()->first + 1;
        }
        // the scalars the open derives: the staged job path, the class table, the exact-sum guard, the batch path
        prep.fast_ok = (core->cfg.engine_mode == 2 || prep.n_relpipe > 0) ? 0 : 1;
        const std::vector<ClassRec> old_classes = prep.classes; const std::vector<int> old_remap = prep.remap;
        if (prep.keyed) prep.rank_classes(core->cfg, sp.any);
        remap_changed = prep.remap != old_remap;
        cls_changed = prep.classes.size() != old_classes.size() || (!prep.classes.empty() && std::memcmp(prep.classes.data(), old_classes.data(), prep.classes.size() * sizeof(ClassRec)) != 0);
        if (dl->node_allocatable && NN) prep.exact_sums = prep.eval_exact_sums(R);  // (only node rows move the guard: the pods' requests are the snapshot's)
        prep.batch_ok = core->cfg.engine_mode == 0 && R <= 4 && prep.n_heights <= 16 && prep.exact_sums;
        // the rows: the clock, and the queues' shares as the open of S' builds them (the only thing the host preparation derives from the rows)
        if (rw && (rw->fields & KAI_ROWS_HAS_NOW)) { core->cfg.now_ns = rw->now_ns; c.now_ns = rw->now_ns; }
        for (int i = 0; i < NQ; i++) for (int k = 0; k < 3; k++) {
            QShare& x = prep.shares[(size_t)rw->queue[i] * 3 + k]; const size_t at = (size_t)k * NQ + i;
            if (rw->queue_deserved) x.deserved = kd_quota_row(k, rw->queue_deserved[at]);
            if (rw->queue_limit) x.max_allowed = kd_quota_row(k, rw->queue_limit[at]);
            if (rw->queue_oqw) x.oqw = rw->queue_oqw[at];
            if (rw->queue_usage) x.usage = rw->queue_usage[at];
        }
    }
    // ---- (5a) the device: k_apply_delta scatters into the baselines (the legacy-MIG nodes outside the delta as a second, small copy), k_apply_rows beside it
    int scatter() {
        const int NX = NN + (int)extra.size();
        int32_t* dnode = reinterpret_cast<int32_t*>(dv) + 4 * NP; uint32_t* dflags = reinterpret_cast<uint32_t*>(dv) + 4 * NP + NN;
        if (!touched.empty()) {  // legacy-MIG bits changed: the node section again, with the nodes outside the delta behind the delta's ([node NX][flags NX], [R][NX]; NX <= NNcap)
            dflags = reinterpret_cast<uint32_t*>(dv) + 4 * NP + NX;
            std::vector<int32_t> nid((size_t)NX); std::vector<uint32_t> nfl((size_t)NX); std::vector<double> nal((size_t)R * NX);
            for (int k = 0; k < NX; k++) {
                const int e = k < NN ? eng[(size_t)k] : extra[(size_t)(k - NN)];
                nid[(size_t)k] = prep.perm[(size_t)e]; nfl[(size_t)k] = prep.node_flags[(size_t)e];
                for (int r = 0; r < R; r++) nal[(size_t)r * NX + k] = prep.node_alloc[(size_t)r * N + e];
            }
            std::memcpy(h32 + 4 * NP, nid.data(), (size_t)NX * 4); std::memcpy(h32 + 4 * NP + NX, nfl.data(), (size_t)NX * 4); std::memcpy(h64, nal.data(), (size_t)R * NX * 8);
            if (NX) { HIP_TRY(core, hipMemcpyAsync(dnode, h32 + 4 * NP, (size_t)2 * NX * 4, hipMemcpyHostToDevice, core->stream));
                      HIP_TRY(core, hipMemcpyAsync(dv + L.o_f64, h64, (size_t)R * NX * 8, hipMemcpyHostToDevice, core->stream)); }
        }
        v.node = dnode; v.node_flags = dflags; v.n_nodes = NX;
        if (NP + NX) hipLaunchKernelGGL(k_apply_delta, dim3((NP + NX + KD_TB - 1) / KD_TB), dim3(KD_TB), 0, core->stream, v, core->d_status0, core->d_node0, core->aux.group0,
                                        (double*)KAI_VP(c.n_alloc), (uint32_t*)KAI_VP(c.n_flags));
        HIP_TRY(core, hipGetLastError());
        if (NQ + NJ) {
            // an array that was NULL at the open and gets its first rows: S' has it, with the value an absent array stands for in every other row.  The context points at a
            // new array from here on (mr_on() switches on the presence of j_last_start), and the victim actions' replicas are laid out again, as when the class table grows.
            auto fresh = [&](auto& field, size_t n, int byte) { core->mw_world = 0; return dfill_f(core, field, n, byte); };
            if (rv.last_start && !c.j_last_start) KAI_TRY(fresh(c.j_last_start, (size_t)c.J, 0));
            if (rv.preempt_mr && !c.q_preempt_mr) KAI_TRY(fresh(c.q_preempt_mr, (size_t)c.Q, 0xFF));
            if (rv.reclaim_mr && !c.q_reclaim_mr) KAI_TRY(fresh(c.q_reclaim_mr, (size_t)c.Q, 0xFF));
            hipLaunchKernelGGL(k_apply_rows, dim3((NQ + NJ + KD_TB - 1) / KD_TB), dim3(KD_TB), 0, core->stream, rv, core->d_shares0, (int32_t*)KAI_VP(c.q_prio),
                               (int64_t*)KAI_VP(c.q_preempt_mr), (int64_t*)KAI_VP(c.q_reclaim_mr), (int64_t*)KAI_VP(c.j_last_start));
            HIP_TRY(core, hipGetLastError());
        }
        return KAI_OK;
    }
    // ---- (5b) the class labels if the table changed, the context's scalars as the open sets them, the session math re-derived as kai_session_reset does
    int rederive() {
        if (cls_changed || remap_changed) {
            const int C = (int)prep.classes.size();
            if (C > core->cls_cap) {  // more classes than the session's arrays hold: new ones for KAI_CMAX (the victim actions' replicas are laid out again)
                KAI_TRY(dalloc_f(core, c.cls, (size_t)KAI_CMAX));
                KAI_TRY(dzero_f(core, c.sum1_key, (size_t)KAI_CMAX * std::max(c.NB, 1))); KAI_TRY(dzero_f(core, c.sum1_node, (size_t)KAI_CMAX * std::max(c.NB, 1)));
                core->cls_cap = KAI_CMAX; core->mw_world = 0;
            }
            if (C) HIP_TRY(core, hipMemcpyAsync(KAI_VP(c.cls), prep.classes.data(), (size_t)C * sizeof(ClassRec), hipMemcpyHostToDevice, core->stream));
            c.C = C;
        }
        if (remap_changed && P) {
            if (!core->d_pkey) {  // the pods' request keys, once per session
                int32_t* t = nullptr; KAI_TRY(dalloc(core, &t, (size_t)P));
                HIP_TRY(core, hipMemcpyAsync(t, prep.pod_key.data(), (size_t)P * 4, hipMemcpyHostToDevice, core->stream)); core->d_pkey = t;
            }
            if (prep.remap.size() > core->remap_cap) { int32_t* t = nullptr; KAI_TRY(dalloc(core, &t, prep.remap.size())); core->d_remap = t; core->remap_cap = prep.remap.size(); }
            std::vector<int32_t> rm(prep.remap.begin(), prep.remap.end());
            if (!rm.empty()) HIP_TRY(core, hipMemcpyAsync(core->d_remap, rm.data(), rm.size() * 4, hipMemcpyHostToDevice, core->stream));
            hipLaunchKernelGGL(k_class_remap, dim3((P + KD_TB - 1) / KD_TB), dim3(KD_TB), 0, core->stream, P, (const int32_t*)core->d_pkey, (const uint8_t*)KAI_VP(c.p_shared), sp.any ? 1 : 0,
                               (const int32_t*)core->d_remap, (int32_t*)KAI_VP(c.p_scls));
            HIP_TRY(core, hipGetLastError());
            HIP_TRY(core, hipStreamSynchronize(core->stream));  // (rm dies with this scope)
        }
        if (core->shared) {  // each node's active pods, flattened (a session with shared-GPU requests: O(nodes + active pods))
            std::vector<int32_t> np_off((size_t)N + 1, 0), np_pods;
            for (int n = 0; n < N; n++) np_off[(size_t)n + 1] = np_off[(size_t)n] + (int32_t)core->np_lists[(size_t)n].size();
            np_pods.reserve((size_t)np_off[(size_t)N]);
            for (int n = 0; n < N; n++) for (const auto& x : core->np_lists[(size_t)n]) np_pods.push_back(x.second);
            if (np_pods.size() > core->np_cap) { int32_t* t = nullptr; KAI_TRY(dalloc(core, &t, np_pods.size())); core->aux.np_pods = t; core->np_cap = np_pods.size(); }
            HIP_TRY(core, hipMemcpyAsync(core->aux.np_off, np_off.data(), np_off.size() * 4, hipMemcpyHostToDevice, core->stream));
            if (!np_pods.empty()) HIP_TRY(core, hipMemcpyAsync(core->aux.np_pods, np_pods.data(), np_pods.size() * 4, hipMemcpyHostToDevice, core->stream));
            HIP_TRY(core, hipStreamSynchronize(core->stream));
        }
        // the context's scalars as the open sets them from the snapshot
        c.use_index = (c.C > 0 && !core->idx_forced_off) ? 1 : 0;
        c.all_tracked = (core->shared || sp.mig) ? 0 : prep.all_tracked;
        core->fast_ok0 = core->fast_forced_off ? 0 : prep.fast_ok; c.fast_ok = core->fast_ok0;
        c.exact_sums = prep.exact_sums;
        {   const bool want = prep.batch_ok && c.use_index && c.all_tracked && c.fast_ok && c.R <= 4 && (c.plugins & KAI_PLUGIN_PROPORTION) && !core->shared;
            if (!want) c.bt.enabled = 0;
            else if (core->bt_alloc && core->bt_C >= c.C) { c.bt = core->bt_pools; c.bt.enabled = 1; }
            else {
                KAI_TRY(bind_batch_pools(core));
                HIP_TRY(core, hipStreamSynchronize(core->stream));  // (the tables batch_bind uploads are the handle's host prep: stable, but keep the order plain)
            }
        }
        KAI_TRY(reset_state(core));
        HIP_TRY(core, hipMemcpyAsync(core->d_ctx, &core->ctx, sizeof(KaiCtx), hipMemcpyHostToDevice, core->stream));
        HIP_TRY(core, hipStreamSynchronize(core->stream));
        core->err = "ok";
        return KAI_OK;
    }
};

int update_impl(kai_core* core, const kai_session_delta* dl, const kai_session_rows* rw, bool& wrote) {
    const bool prof = std::getenv("KAI_PROF") != nullptr;  // host clocks of the update (stderr), as kai_session_open reports its own
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(core, hipSetDevice(core->device));
    SessionUpdate u(core, dl, rw);
    KAI_TRY(u.stage_and_gather());
    KAI_TRY(u.refusals());
    wrote = true;  // from here on the session's own state changes: a failure closes the session (session_update)
    const auto t1 = std::chrono::steady_clock::now();
    u.host_bookkeeping();
    const auto t2 = std::chrono::steady_clock::now();
    KAI_TRY(u.scatter());
    KAI_TRY(u.rederive());
    if (prof) { const auto t3 = std::chrono::steady_clock::now(); std::fprintf(stderr, "kai update: %d pods %d nodes %d queue rows %d job rows | stage + gather + checks %.3f, host bookkeeping %.3f, device (scatter, classes, re-derivation) %.3f | total %.3f ms\n",
                             u.NP, u.NN, u.NQ, u.NJ, ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, t3), ms_between(t0, t3)); }
    return KAI_OK;
}

// the arguments of both parts, checked on the host before anything is written or sent (what: the entry point's name, for the messages)
int check_update_args(kai_core* core, const kai_session_delta* d, const kai_session_rows* r, const std::string& what) {
    auto bad = [&](const char* m) { core->err = what + ": " + m; return (int)KAI_ERR_INVALID_ARG; };
    const int N = core->ctx.N, P = core->ctx.P, J = core->ctx.J, Q = core->ctx.Q;
    auto twice = [](const int32_t* x, int n) { std::vector<int32_t> a(x, x + n); std::sort(a.begin(), a.end()); return std::adjacent_find(a.begin(), a.end()) != a.end(); };
    if (d) {
        if (d->version != KAI_DELTA_VERSION) return bad("wrong delta version");
        const int NP = d->n_pods, NN = d->n_nodes;
        if (NP < 0 || NN < 0) return bad("negative count");
        if (NP > 0 && (!d->pod || !d->pod_status || !d->pod_node)) return bad("a required pod array is NULL");
        if (NN > 0 && !d->node) return bad("the node array is NULL");
        for (int i = 0; i < NP; i++) {
            if (d->pod[i] < 0 || d->pod[i] >= P) return bad("pod index out of range");
            if (d->pod_node[i] < -1 || d->pod_node[i] >= N) return bad("pod_node out of range");
        }
        for (int k = 0; k < NN; k++) if (d->node[k] < 0 || d->node[k] >= N) return bad("node index out of range");
        if (twice(d->pod, NP)) return bad("a pod is listed twice");
        if (twice(d->node, NN)) return bad("a node is listed twice");
    }
    if (r) {  // (the open reads the rows' values as they are — it refuses none of them — so there is nothing to refuse in a value here either)
        if (r->version != KAI_ROWS_VERSION) return bad("wrong rows version");
        if (r->fields & ~KAI_ROWS_HAS_NOW) return bad("unknown bits in rows.fields");
        const int NQ = r->n_queues, NJ = r->n_jobs;
        if (NQ < 0 || NJ < 0) return bad("negative count");
        if (NQ > 0 && !r->queue) return bad("the queue index array is NULL");
        if (NJ > 0 && !r->job) return bad("the job index array is NULL");
        for (int i = 0; i < NQ; i++) if (r->queue[i] < 0 || r->queue[i] >= Q) return bad("queue index out of range");
        for (int i = 0; i < NJ; i++) if (r->job[i] < 0 || r->job[i] >= J) return bad("job index out of range");
        if (twice(r->queue, NQ)) return bad("a queue is listed twice");
        if (twice(r->job, NJ)) return bad("a job is listed twice");
    }
    return KAI_OK;
}

int session_update(kai_core* core, const kai_session_delta* d, const kai_session_rows* r, const char* what) {
    if (!core->open) return fail(core, KAI_ERR_STATE, "no open session");
    if (core->world > 1) { core->err = std::string(what) + ": a handle of a sharded group (open the new snapshot on every rank)"; return KAI_ERR_UNSUPPORTED; }
    static const kai_session_delta no_delta = {KAI_DELTA_VERSION, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr};
    bool wrote = false;
    const int rc = no_throw(core, what, [&] { const int rca = check_update_args(core, d, r, what); return rca ? rca : update_impl(core, d ? d : &no_delta, r, wrote); });
    if (rc != KAI_OK && wrote) close_failed(core);  // the writes began: the session is no longer the snapshot it was, nor S' — closed, as a failed open leaves it
    else if (rc != KAI_OK && core->stream) (void)hipStreamSynchronize(core->stream);
    if (rc == KAI_OK) core->st_open = false;  // the update drops an open Statement (kai_stmt.hpp) with the action results
    return rc;
}
}  // namespace
