// subset_nodes_sim.cpp — TEST INFRASTRUCTURE: kai_subset_nodes' kernel bodies and control flow (kai-scheduler_amd/csrc/kai_subset_nodes.hpp: sn_count with sn_tta_body, sn_prep_body,
// sn_wide_body / sn_engine_walk, sn_offsets_body, then sn_emit_body) compiled with plain g++ and run with the emulated lanes of kai_simt.hpp on a session of the host simulation
// (sim_session.hpp: struct SimSession).  tests/test_subset_nodes.py compares the node sets with the oracle's subSetNodesFn (kai_oracle_subset_nodes_all) and the session with a TWIN
// that never made the call.  NOT a CPU fallback: libkai_core never contains it; the parity claim is tests/test_gpu_subset_nodes.py on the MI355X.
//
// The harness: open the session; run the actions `pre`; copy the state; make the call on its context; compare the state with the copy; run the actions `post`; read back.
//
// -DKAI_SNSIM_MAIN adds a main() with one fixed case (the stand-alone program the sanitizers are run on).
#include "sim_session.hpp"
#include "../../kai-scheduler_amd/csrc/kai_subset_nodes.hpp"

namespace {

// the handle's scratch and the emitted sets' buffer: grow, keep what the last call left
struct SnScratch { std::vector<unsigned char> dev, out; bool tab_ok = false; };

struct SnSimLauncher {
    int launches = 0, reads = 0;
    void tta(int g, int b, const KaiCtx& c, const SnArgs& a) { launches++; kw::launch(g, b, 0, [&] { sn_tta_body(c, a); }); }
    void prep(int g, int b, const KaiCtx& c, const SnArgs& a) { launches++; kw::launch(g, b, 0, [&] { sn_prep_body(c, a); }); }
    void wide(int g, int b, const KaiCtx& c, const SnArgs& a) { launches++; kw::launch(g, b, 0, [&] { sn_wide_body(c, a); }); }
    void offsets(int g, int b, const KaiCtx& c, const SnArgs& a) { launches++; kw::launch(g, b, 0, [&] { sn_offsets_body(c, a); }); }
    void emit(int g, int b, const KaiCtx& c, const SnArgs& a) { launches++; kw::launch(g, b, 0, [&] { sn_emit_body(c, a); }); }
    int engine(const KaiCtx& c, const SnArgs& a) { launches++; NullBackend be; sn_engine_walk(c, be, a); return 0; }  // as k_sn_engine: one lane, no scan lanes
    int read_head(SnHead& hd, const SnArgs& a) { reads++; hd = *a.head; return 0; }
};

// kai_subset_nodes from its first device call on (the refusals in front of it are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp) -> what the entry point
// would return.  wgs: workgroups of the chip-wide walk and of the emit (fewer than the queries / records: the grid-stride loops).
int sim_subset_nodes(SimSession& ss, SnScratch& sc, uint32_t flags, int lanes, int wgs, const kai_subset_query* queries, int M, const uint32_t* rows_in, int S,
                     kai_subset_answer* answers_out, kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out, uint32_t* bitmaps_out, kai_subset_result& res) {
    const KaiCtx& c = ss.ctx();
    const HostPrep& hp = ss.prep;
    const int N = c.N, W = (N + 31) / 32, DT = c.D + c.T;
    if (M == 0) { *n_sets_out = 0; res.n_sets = 0; res.path = KAI_SUBSET_PATH_NONE; res.pad = 0; return KAI_OK; }
    std::vector<int> cnt((size_t)std::max(c.T, 1), 1);
    for (int d = 0; d < c.D; d++) cnt[(size_t)hp.dom_topo[(size_t)d]]++;
    int stride = 1, levels = 0;
    for (int t = 0; t < c.T; t++) { stride = std::max(stride, cnt[(size_t)t]); levels = std::max(levels, hp.topo_level_off[(size_t)t + 1] - hp.topo_level_off[(size_t)t]); }
    const bool wide = !(flags & KAI_SUBSET_ENGINE_PATH) && sn_wide_session(c, levels);
    const int n_wgs = wide ? std::max(1, std::min(M, wgs)) : 0, n_children = DT > 0 ? hp.dom_child_off[(size_t)DT] : 0;
    const SnLayout L(N, M, S, W, stride, DT, n_children, n_wgs);
    if (sc.dev.size() < L.end) { sc.dev.assign(L.end + L.end / 4, 0xA5); sc.tab_ok = false; }  // (no kernel may read what it did not write)
    unsigned char* d = sc.dev.data();
    if (!sc.tab_ok) {
        int32_t* rank = reinterpret_cast<int32_t*>(d + L.rank);
        if (N > 0) std::memcpy(d + L.perm, hp.perm.data(), (size_t)N * 4);
        for (int i = 0; i < N; i++) rank[hp.perm[(size_t)i]] = i;
        if (n_children > 0) std::memcpy(d + L.children, hp.dom_children.data(), (size_t)n_children * 4);
        sc.tab_ok = true;
    }
    std::memcpy(d + L.queries, queries, (size_t)M * sizeof(kai_subset_query));
    if (S > 0 && W > 0) std::memcpy(d + L.rows_in, rows_in, (size_t)S * W * 4);
    std::memset(d + L.head, 0, sizeof(SnHead));
    SnArgs a = sn_bind_args(d, L, M, S, W, stride);
    a.want_bitmaps = bitmaps_out ? 1 : 0;
    KaiCtx cq = c; cq.action = KAI_ACTION_ALLOCATE;
    SnSimLauncher l; SnHead hd{}; int path = KAI_SUBSET_PATH_NONE;
    if (int rc = sn_count(l, cq, a, wide, lanes, n_wgs, hd, path)) return rc;
    const int64_t total = hd.total;
    if (total > sets_cap) { *n_sets_out = total; return KAI_ERR_CAPACITY; }
    const size_t set_bytes = (size_t)total * sizeof(kai_node_set), map_bytes = bitmaps_out ? (size_t)total * W * 4 : 0;
    if (total > 0) {
        sc.out.assign(set_bytes + map_bytes + 16, 0xA5);
        a.sets = (kai_node_set*)sc.out.data(); a.bitmaps = (uint32_t*)(sc.out.data() + set_bytes);
        l.emit((int)std::min<int64_t>(total, std::max(1, wgs)), lanes, cq, a);
        std::memcpy(sets_out, sc.out.data(), set_bytes);
        if (bitmaps_out) std::memcpy(bitmaps_out, sc.out.data() + set_bytes, map_bytes);
    }
    std::memcpy(answers_out, d + L.answers, (size_t)M * sizeof(kai_subset_answer));
    *n_sets_out = total;
    res.n_sets = total; res.path = path; res.pad = 0;
    return KAI_OK;
}

// what the call may re-derive (include/kai_core.h): the tasks-to-allocate caches' validity is the one word of StateCopy::hidden it may change
void mask_rederived(const KaiCtx& c, StateCopy& g) { for (int j = 0; j < c.J; j++) g.hidden[(size_t)4 * c.P + (size_t)4 * c.S + (size_t)8 * j + 1] = 0; }
bool same_state(const StateCopy& a, const StateCopy& b) {
    return a.p_status == b.p_status && a.p_node == b.p_node && a.hidden == b.hidden && a.n_idle.size() == b.n_idle.size() && a.shares.size() == b.shares.size() &&
           std::memcmp(a.n_idle.data(), b.n_idle.data(), a.n_idle.size() * 8) == 0 && std::memcmp(a.n_rel.data(), b.n_rel.data(), a.n_rel.size() * 8) == 0 &&
           std::memcmp(a.n_used.data(), b.n_used.data(), a.n_used.size() * 8) == 0 && std::memcmp(a.shares.data(), b.shares.data(), a.shares.size() * sizeof(QShare)) == 0;
}

}  // namespace

extern "C" {

// Runs the actions `pre`, then — mode 0 — kai_subset_nodes with `flags` for the M queries over the S parent rows in workgroups of `lanes` lanes and grids of at most `wgs`
// workgroups (mode 1: no call, the twin), then the actions `post`.  call_status: what the entry point would return.  *unchanged: the state right behind the call (read-backs,
// the state no read-back shows, the action statistics, fast_ok, the class index's staleness, the engine's scalars) is the state right in front of it.  ops_out ...: the
// operations of ALL actions and the final pod state, as kai_hostsim_run returns them.
int kai_snsim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* pre, int n_pre, int batch, int mode, uint32_t flags, int lanes, int wgs,
                  const kai_subset_query* queries, int M, const uint32_t* rows_in, int S, kai_subset_answer* answers_out, kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out,
                  uint32_t* bitmaps_out, kai_subset_result* result, int* call_status, int* unchanged,
                  const int* post, int n_post, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out) {
    if (!cfg || !s || n_pre < 0 || n_post < 0 || lanes < 1 || lanes > 4096 || wgs < 1 || M < 0 || S < 0 || (mode != 0 && mode != 1) || (mode == 0 && (!n_sets_out || sets_cap < 0))) return KAI_ERR_INVALID_ARG;
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_pre + n_post, batch != 0)) return rc;
    for (int i = 0; i < n_pre; i++) if (int rc = ss.action(pre[i])) return rc;
    SnScratch scratch; int status = KAI_OK; kai_subset_result res{}; int same = 1;
    if (mode == 0) {
        StateCopy before = ss.snapshot_state(); kai_action_stats st0{}, st1{}; ss.stats(&st0);
        const int fast0 = ss.ctx().fast_ok, act0 = ss.ctx().action; const bool stale0 = ss.index_stale; const EngineState es0 = *ss.ctx().st;
        status = sim_subset_nodes(ss, scratch, flags, lanes, wgs, queries, M, rows_in, S, answers_out, sets_out, sets_cap, n_sets_out, bitmaps_out, res);
        StateCopy after = ss.snapshot_state(); ss.stats(&st1);
        mask_rederived(ss.ctx(), before); mask_rederived(ss.ctx(), after);
        same = same_state(before, after) && std::memcmp(&st0, &st1, sizeof st0) == 0 && fast0 == ss.ctx().fast_ok && act0 == ss.ctx().action && stale0 == ss.index_stale &&
               std::memcmp(&es0, ss.ctx().st, sizeof es0) == 0;
    }
    for (int i = 0; i < n_post; i++) if (int rc = ss.action(post[i])) return rc;
    if (int rc = ss.finish()) return rc;
    if (call_status) *call_status = status;
    if (result) *result = res;
    if (unchanged) *unchanged = same;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops)) return rc;
    ss.pod_state(pod_status_out, pod_node_out);
    return KAI_OK;
}

}  // extern "C"

#ifdef KAI_SNSIM_MAIN
// One fixed case: 2 zones x 3 racks x 4 nodes of 8 GPUs (name ranks the reverse of the indices), two nodes without labels; one queue; pending gangs of one to six one- or
// two-GPU pods whose root groups require the zone and prefer the rack, require the rack, or only prefer it; a few running pods fill the racks unevenly.  The call with 256, 100
// and 1 lanes and grids of 3 and many workgroups, both paths, fresh and behind an allocate: the two paths agree record for record and word for word, `first` is the running sum,
// every set's bitmap row holds n_nodes nodes of the parent row and of the set's domain, the session is as it was, a capacity below the count reports the count and writes
// nothing, and the next allocate commits what the twin's commits.
int main() {
    const int Z = 2, RK = 3, PER = 4, N = Z * RK * PER + 2, NJ = 18, RUN = 5, J = NJ + RUN, R = 4, Q = 1, D = Z + Z * RK;
    std::vector<int32_t> jnp(J), jfp(J), jq(J, 0), jprio(J), jpre(J, 1), jfps(J), jnps(J, 1); std::vector<int64_t> jcreated(J); std::vector<uint32_t> juid(J);
    int P = 0;
    for (int j = 0; j < J; j++) { jnp[j] = j < NJ ? 1 + j % 6 : 3; jfp[j] = P; P += jnp[j]; jprio[j] = 50 + j % 2; jfps[j] = j; juid[j] = (uint32_t)j; jcreated[j] = 1000 + j; }
    const int S = J;
    std::vector<double> alloc((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> nflags(N, 0u), nrank(N), pflags(P, 0u), puid(P), quid(Q, 0u), psrank(S, 0u);
    std::vector<int32_t> ngc(N, -1), ncls(N, 0), pjob(P), pps(P), pst(P), pnode(P), pprio(P, 0), pcls(P, 0), pnom(P, -1), psjob(S), psmin(S), qpar = {-1}, qprio = {0};
    std::vector<int64_t> pcreated(P), qcreated(Q, 10);
    for (int n = 0; n < N; n++) { nrank[n] = (uint32_t)(N - 1 - n); alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256000; alloc[2 * N + n] = 8; alloc[3 * N + n] = 110; }
    for (int j = 0; j < J; j++) { psjob[j] = j; psmin[j] = jnp[j]; }
    for (int p = 0, j = 0; p < P; p++) {
        while (p >= jfp[j] + jnp[j]) j++;
        pjob[p] = j; pps[p] = j; puid[p] = (uint32_t)p; pcreated[p] = 2000 + p;
        const bool running = j >= NJ;
        pst[p] = running ? KAI_POD_RUNNING : KAI_POD_PENDING; pnode[p] = running ? (p * 5) % (Z * RK * PER) : -1;
        req[0 * P + p] = 1000; req[1 * P + p] = 4000; req[2 * P + p] = running ? 3 : j % 9 == 4 ? 9 : 1 + j % 2;  // (9 GPUs: more than a node has) req[3 * P + p] = 1;
    }
    // the topology: level 0 = zone (domains 0 .. Z-1), level 1 = rack (domains Z ..), the last two nodes outside it
    std::vector<int32_t> topo_off = {0, 2}, ndom((size_t)2 * N, -1), dpar(D), dlvl(D); std::vector<uint32_t> drank(D);
    for (int n = 0; n < Z * RK * PER; n++) { const int z = n / (RK * PER), rk = n / PER; ndom[0 * N + n] = z; ndom[1 * N + n] = Z + rk; }
    for (int d = 0; d < D; d++) { dpar[d] = d < Z ? -1 : (d - Z) / RK; dlvl[d] = d < Z ? 0 : 1; drank[d] = (uint32_t)(D - 1 - d); }
    std::vector<int32_t> gjob(J), gpar(J, -1), gtopo(J, 0), greq(J), gpref(J), jroot(J), sgrp(S), stopo(S, -1), sreq(S, -1), spref(S, -1); std::vector<uint32_t> grank(J, 0u);
    for (int j = 0; j < J; j++) { gjob[j] = j; jroot[j] = j; sgrp[j] = j; greq[j] = j % 3 == 0 ? 0 : j % 3 == 1 ? 1 : -1; gpref[j] = j % 3 == 1 ? -1 : 1; if (j >= NJ) gtopo[j] = -1; }
    std::vector<double> qdes((size_t)3 * Q), qlim((size_t)3 * Q, -1.0), qoqw((size_t)3 * Q, 1.0);
    qdes[0] = 1e6; qdes[1] = 1e6; qdes[2] = 200;
    const uint8_t fit = 1;
    kai_snapshot_soa s; std::memset(&s, 0, sizeof s);
    s.abi_version = KAI_ABI_VERSION; s.n_res = R;
    s.n_nodes = N; s.node_allocatable = alloc.data(); s.node_flags = nflags.data(); s.node_gpu_count = ngc.data(); s.node_name_rank = nrank.data(); s.node_class = ncls.data();
    s.n_pods = P; s.pod_req = req.data(); s.pod_job = pjob.data(); s.pod_podset = pps.data(); s.pod_status = pst.data(); s.pod_node = pnode.data(); s.pod_flags = pflags.data();
    s.pod_task_priority = pprio.data(); s.pod_created_ns = pcreated.data(); s.pod_uid_rank = puid.data(); s.pod_class = pcls.data(); s.pod_nominated_node = pnom.data();
    s.n_podsets = S; s.podset_job = psjob.data(); s.podset_min_available = psmin.data(); s.podset_name_rank = psrank.data();
    s.n_jobs = J; s.job_queue = jq.data(); s.job_priority = jprio.data(); s.job_preemptible = jpre.data(); s.job_created_ns = jcreated.data(); s.job_uid_rank = juid.data();
    s.job_first_pod = jfp.data(); s.job_n_pods = jnp.data(); s.job_first_podset = jfps.data(); s.job_n_podsets = jnps.data();
    s.n_queues = Q; s.queue_parent = qpar.data(); s.queue_priority = qprio.data(); s.queue_created_ns = qcreated.data(); s.queue_uid_rank = quid.data();
    s.queue_deserved = qdes.data(); s.queue_limit = qlim.data(); s.queue_oqw = qoqw.data();
    s.n_pod_classes = 1; s.n_node_classes = 1; s.class_fit = &fit;
    s.n_topologies = 1; s.n_topo_levels = 2; s.topo_level_off = topo_off.data(); s.node_domain = ndom.data(); s.n_domains = D; s.domain_level = dlvl.data(); s.domain_parent = dpar.data(); s.domain_id_rank = drank.data();
    s.n_groups = J; s.group_job = gjob.data(); s.group_parent = gpar.data(); s.group_name_rank = grank.data(); s.group_topology = gtopo.data(); s.group_required_level = greq.data();
    s.group_preferred_level = gpref.data(); s.job_root_group = jroot.data(); s.podset_group = sgrp.data(); s.podset_topology = stopo.data(); s.podset_required_level = sreq.data();
    s.podset_preferred_level = spref.data();
    kai_config cfg; std::memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = KAI_ABI_VERSION; cfg.k_value = 1.0; cfg.reclaimer_saturation_multiplier = 1.0; cfg.plugins = KAI_PLUGIN_ALL; cfg.max_consolidation_preemptees = 16;
    cfg.allow_consolidating_reclaim = 1; cfg.full_hierarchy_fairness = 1; cfg.min_node_gpu_memory = 100; for (int i = 0; i < 4; i++) cfg.queue_depth[i] = -1;
    cfg.now_ns = 1;

    const int W = (N + 31) / 32, NS = 2;
    std::vector<uint32_t> rows((size_t)NS * W, 0u);
    for (int n = 0; n < N; n++) { if (n % 3 != 1) rows[0 * W + (n >> 5)] |= 1u << (n & 31); if (n >= RK * PER) rows[1 * W + (n >> 5)] |= 1u << (n & 31); }  // a sparse row; zone 1 and the unlabelled nodes
    std::vector<kai_subset_query> qs;
    for (int j = 0; j < J; j++) for (int row = -1; row < NS; row++) { kai_subset_query q; q.job = j; q.group = row == 0 ? j : -1; q.podset = -1; q.nodeset = row; qs.push_back(q); }
    const int M = (int)qs.size(); const int64_t CAP = (int64_t)M * (D + 2);

    struct Out { int rc = 99, status = 99, same = 0; kai_subset_result res{}; std::vector<kai_subset_answer> ans; std::vector<kai_node_set> sets; std::vector<uint32_t> maps; int64_t n = -3; std::vector<kai_op> ops; std::vector<int32_t> st, nd; };
    const int ALLOC[1] = {KAI_ACTION_ALLOCATE};
    auto run = [&](bool pre, int mode, uint32_t flags, int lanes, int wgs, int64_t cap, bool post, Out& o) {
        kai_subset_answer pa; std::memset(&pa, 0x77, sizeof pa); kai_node_set pz; std::memset(&pz, 0x77, sizeof pz);
        o.ans.assign((size_t)M, pa); o.sets.assign((size_t)CAP, pz); o.maps.assign((size_t)CAP * W, 0x77777777u); o.st.assign(P, 0); o.nd.assign(P, 0); o.ops.assign((size_t)8 * P + 64, kai_op{}); int64_t nops = 0;
        o.rc = kai_snsim_run(&cfg, &s, pre ? ALLOC : nullptr, pre ? 1 : 0, 0, mode, flags, lanes, wgs, qs.data(), M, rows.data(), NS, o.ans.data(), o.sets.data(), cap, &o.n, o.maps.data(), &o.res,
                             &o.status, &o.same, post ? ALLOC : nullptr, post ? 1 : 0, o.ops.data(), (int64_t)o.ops.size(), &nops, o.st.data(), o.nd.data());
        o.ops.resize((size_t)nops);
        return o.rc;
    };
    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what) { checks++; if (!ok) { bad++; std::printf("FAILED: %s\n", what); } };
    auto consistent = [&](const Out& o) {
        int64_t run_sum = 0;
        for (int i = 0; i < M; i++) {
            const kai_subset_answer& a = o.ans[(size_t)i];
            if (a.first != run_sum || a.n_sets < 0 || a.pad != 0 || (a.status == KAI_SUBSET_OK) != (a.n_sets > 0)) return false;
            for (int k = 0; k < a.n_sets; k++) {
                const kai_node_set& z = o.sets[(size_t)(a.first + k)]; const uint32_t* m = &o.maps[(size_t)(a.first + k) * W];
                int cnt = 0;
                for (int n = 0; n < N; n++) {
                    if (!((m[n >> 5] >> (n & 31)) & 1u)) continue;
                    cnt++;
                    if (qs[(size_t)i].nodeset >= 0 && !((rows[(size_t)qs[(size_t)i].nodeset * W + (n >> 5)] >> (n & 31)) & 1u)) return false;
                    if (z.domain >= 0 && ndom[(size_t)z.level * N + n] != z.domain) return false;
                    if (z.domain <= KAI_SUBSET_ROOT(0) && ndom[n] < 0) return false;
                }
                if (cnt != z.n_nodes) return false;
            }
            run_sum += a.n_sets;
        }
        return run_sum == o.n && o.res.n_sets == o.n;
    };
    auto equal = [&](const Out& x, const Out& y) {
        return x.n == y.n && std::memcmp(x.ans.data(), y.ans.data(), (size_t)M * sizeof(kai_subset_answer)) == 0 && std::memcmp(x.sets.data(), y.sets.data(), (size_t)x.n * sizeof(kai_node_set)) == 0 &&
               std::memcmp(x.maps.data(), y.maps.data(), (size_t)x.n * W * 4) == 0;
    };
    for (bool pre : {false, true}) {
        Out first; bool have = false;
        for (int lanes : {256, 100, 1}) for (int wgs : {3, 1 << 20}) {
            if (lanes == 1 && wgs == 3) continue;
            Out w, e;
            expect(run(pre, 0, 0, lanes, wgs, CAP, false, w) == 0 && w.status == KAI_OK && w.res.path == KAI_SUBSET_PATH_WIDE, "the call on the chip-wide path");
            expect(run(pre, 0, KAI_SUBSET_ENGINE_PATH, lanes, wgs, CAP, false, e) == 0 && e.status == KAI_OK && e.res.path == KAI_SUBSET_PATH_ENGINE, "the call on the engine path");
            expect(consistent(w) && consistent(e), "answers, records and bitmap rows belong together");
            expect(equal(w, e), "the two paths agree");
            expect(w.same && e.same, "the call changes nothing");
            if (!have) { first = w; have = true; } else expect(equal(w, first), "every workgroup size and grid: the same answer");
        }
        int lens[3] = {0, 0, 0};
        for (int i = 0; i < M; i++) { const int n = first.ans[(size_t)i].n_sets; lens[n == 0 ? 0 : n == 1 ? 1 : 2]++; }
        if (!pre) expect(lens[0] > 0 && lens[1] > 0 && lens[2] > 0, "empty, single and longer lists all occur");
        else expect(lens[2] == 0 && lens[1] > 0, "behind an allocate every gang that fits is placed: no task, the parent set as it is");
        Out small; expect(run(pre, 0, 0, 256, 8, first.n - 1, false, small) == 0 && small.status == KAI_ERR_CAPACITY && small.n == first.n && small.ans[0].pad == 0x77777777 && small.sets[0].domain == 0x77777777 && small.same, "a capacity below the count: the count needed, nothing written");
    }
    {   Out a, b; expect(run(false, 0, 0, 256, 8, CAP, true, a) == 0 && a.status == KAI_OK, "allocate behind the call");
        expect(run(false, 1, 0, 256, 8, CAP, true, b) == 0, "allocate on the twin");
        expect(a.ops.size() == b.ops.size() && !a.ops.empty() && std::memcmp(a.ops.data(), b.ops.data(), a.ops.size() * sizeof(kai_op)) == 0 && a.st == b.st && a.nd == b.nd, "the next allocate commits the same operations");
        Out e; expect(run(false, 0, KAI_SUBSET_ENGINE_PATH, 256, 8, CAP, true, e) == 0 && e.ops.size() == b.ops.size() && std::memcmp(e.ops.data(), b.ops.data(), e.ops.size() * sizeof(kai_op)) == 0 && e.st == b.st, "... behind the engine path too"); }
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "subset_nodes_sim: %d of %d checks FAILED\n" : "subset_nodes_sim: ok (%d checks)\n", bad ? bad : checks, checks);
    return bad ? 1 : 0;
}
#endif
