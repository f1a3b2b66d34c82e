// topo_scores_sim.cpp — TEST INFRASTRUCTURE: kai_subset_nodes_scored and kai_ordered_nodes_scored from their first device call on (kai-scheduler_amd/csrc/kai_subset_nodes.hpp
// with want_scores set, both paths; k_bn_prep, k_bn_range and k_on_scan_scored of kai_ordered_nodes.hpp) compiled with plain g++ and run with the emulated lanes of kai_simt.hpp
// on ONE session of the host simulation that lives across the calls (sim_session.hpp), so that a test can chain them as a caller does: sets and scores, a scored list per pod,
// kai_ops_apply of the chosen operation, the next pod.  subset_nodes_sim.cpp is included for its launcher, its scratch and its "changes nothing" comparison.
// tests/test_topo_scores.py compares the scores with the oracle's calculateNodeScores (kai_oracle_topology_scores).  NOT a CPU fallback: libkai_core never contains it; the
// parity claim is tests/test_gpu_topo_scores.py on the MI355X.
//
// -DKAI_TSSIM_MAIN adds a main() with one fixed case (the stand-alone program a sanitizer build runs).
#include "subset_nodes_sim.cpp"
#include "../../kai-scheduler_amd/csrc/kai_ordered_nodes.hpp"

namespace {

struct TsSession { SimSession ss; SnScratch scratch; ApplyScratch apply; };

// sim_subset_nodes of subset_nodes_sim.cpp with the two outputs of the scored call
int sim_subset_nodes_scored(SimSession& ss, SnScratch& sc, uint32_t flags, int lanes, int wgs, const kai_subset_query* queries, int M, const uint32_t* rows_in, int S,
                            kai_subset_answer* answers_out, kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out, uint32_t* bitmaps_out,
                            kai_topo_score_row* score_rows_out, uint8_t* deciles_out, kai_subset_result& res) {
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
    const SnLayout L(N, M, S, W, stride, DT, n_children, n_wgs, true, c.D);
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
    std::memset(d + L.score_rows, 0xA5, L.end - L.score_rows);  // every row and every decile must be written by the kernels
    SnArgs a = sn_bind_args(d, L, M, S, W, stride);
    a.want_bitmaps = bitmaps_out ? 1 : 0; a.want_scores = 1;
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
    std::memcpy(score_rows_out, d + L.score_rows, (size_t)M * sizeof(kai_topo_score_row));
    if (c.D > 0) std::memcpy(deciles_out, d + L.deciles, (size_t)M * (size_t)c.D);
    *n_sets_out = total;
    res.n_sets = total; res.path = path; res.pad = 0;
    return KAI_OK;
}

}  // namespace

extern "C" {

// A session that lives until kai_tssim_close: cfg and s must stay alive as long.  n_actions: the actions the session will run (one out_ops list for all of them).
void* kai_tssim_open(const kai_config* cfg, const kai_snapshot_soa* s, int n_actions, int* rc_out) {
    TsSession* t = new TsSession();
    const int rc = t->ss.open(cfg, s, n_actions > 0 ? n_actions : 1, false);
    if (rc_out) *rc_out = rc;
    if (rc) { delete t; return nullptr; }
    return t;
}
void kai_tssim_close(void* h) { delete static_cast<TsSession*>(h); }
int kai_tssim_n_domains(void* h) { return static_cast<TsSession*>(h)->ss.ctx().D; }
int kai_tssim_action(void* h, int action) { return static_cast<TsSession*>(h)->ss.action(action); }

// kai_subset_nodes (scored 0) or kai_subset_nodes_scored (scored 1) on the session's current state.  Returns what the entry point would return; *unchanged as kai_snsim_run's.
int kai_tssim_subset(void* h, int scored, uint32_t flags, int lanes, int wgs, const kai_subset_query* queries, int M, const uint32_t* rows_in, int S, kai_subset_answer* answers_out,
                     kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out, uint32_t* bitmaps_out, kai_topo_score_row* score_rows_out, uint8_t* deciles_out,
                     kai_subset_result* result, int* unchanged) {
    if (!h || !n_sets_out || lanes < 1 || lanes > 4096 || wgs < 1 || M < 0 || S < 0 || sets_cap < 0) return KAI_ERR_INVALID_ARG;
    TsSession& t = *static_cast<TsSession*>(h); SimSession& ss = t.ss;
    StateCopy before = ss.snapshot_state(); kai_action_stats st0{}, st1{}; ss.stats(&st0);
    const int fast0 = ss.ctx().fast_ok, act0 = ss.ctx().action; const bool stale0 = ss.index_stale; const EngineState es0 = *ss.ctx().st;
    kai_subset_result res{};
    const int status = scored ? sim_subset_nodes_scored(ss, t.scratch, flags, lanes, wgs, queries, M, rows_in, S, answers_out, sets_out, sets_cap, n_sets_out, bitmaps_out, score_rows_out, deciles_out, res)
                              : sim_subset_nodes(ss, t.scratch, flags, lanes, wgs, queries, M, rows_in, S, answers_out, sets_out, sets_cap, n_sets_out, bitmaps_out, res);
    StateCopy after = ss.snapshot_state(); ss.stats(&st1);
    mask_rederived(ss.ctx(), before); mask_rederived(ss.ctx(), after);
    if (unchanged) *unchanged = same_state(before, after) && std::memcmp(&st0, &st1, sizeof st0) == 0 && fast0 == ss.ctx().fast_ok && act0 == ss.ctx().action && stale0 == ss.index_stale &&
                                std::memcmp(&es0, ss.ctx().st, sizeof es0) == 0;
    if (result) *result = res;
    return status;
}

// kai_ordered_nodes (scored 0: on_scan_body, the fourth word of a query must be 0) or kai_ordered_nodes_scored (scored 1: on_scan_scored_body) on the session's current state.
// lanes: a multiple of 64 up to 256; grid: workgroups of the scan.  out: [M][k], n_out: [M].
int kai_tssim_ordered(void* h, int scored, const kai_scored_query* queries, int M, const uint32_t* rows_in, int S, const kai_topo_score_row* score_rows, const uint8_t* deciles,
                      int n_score_rows, int k, int lanes, int grid, kai_node_answer* out, int32_t* n_out) {
    if (!h || M < 0 || S < 0 || k < 1 || k > KAI_ORDERED_MAX_K || lanes < 64 || lanes > 64 * KAI_ON_MAX_WAVES || lanes % 64 || grid < 1 || n_score_rows < 0) return KAI_ERR_INVALID_ARG;
    SimSession& ss = static_cast<TsSession*>(h)->ss;
    const KaiCtx& c = ss.ctx();
    if (M == 0) return KAI_OK;
    const int W = (c.N + 31) / 32;
    std::vector<uint32_t> rows((size_t)S * W + 1, 0u); std::vector<int32_t> need((size_t)2 * (S + 1), 0); std::vector<double> range((size_t)4 * (S + 1), 0.0);
    std::vector<BnQuery> prep((size_t)M + 1); std::vector<kai_node_answer> unused((size_t)M + 1);
    const kai_node_answer poison = {-7, -7};  // every entry and every length must be written by the kernel
    std::vector<kai_node_answer> lists((size_t)M * k + 1, poison); std::vector<int32_t> lens((size_t)M + 1, -7);
    // the rows as the upload places them: exactly n_score_rows x D bytes, so that a read past a row's end leaves the vector
    std::vector<kai_topo_score_row> srows(score_rows, score_rows + n_score_rows); std::vector<uint8_t> dec(deciles, deciles + (size_t)n_score_rows * c.D);
    BnArgs a; std::memset((void*)&a, 0, sizeof a);
    a.M = M; a.S = S; a.W = W; a.queries = reinterpret_cast<const kai_node_query*>(queries); a.rows_in = rows_in; a.perm = ss.prep.perm.data();
    a.rows = rows.data(); a.need = need.data(); a.range = range.data(); a.prep = prep.data(); a.out = unused.data();
    OnArgs o; std::memset((void*)&o, 0, sizeof o);
    o.k = k; o.out = lists.data(); o.n_out = lens.data();
    OnScoreArgs sa; std::memset((void*)&sa, 0, sizeof sa);
    sa.D = c.D; sa.rows = srows.data(); sa.deciles = dec.data();
    const size_t items = (size_t)M > (size_t)S * W ? (size_t)M : (size_t)S * W;
    kw::launch((int)((items + lanes - 1) / lanes), lanes, 0, [&] { bn_prep_body(c, a); });
    if ((c.plugins & KAI_PLUGIN_NODEPLACEMENT) && (c.gpu_strategy == KAI_BINPACK || c.cpu_strategy == KAI_BINPACK)) kw::launch(2 * (S + 1), lanes, 0, [&] { bn_range_body(c, a); });
    if (scored) kw::launch(grid < M ? grid : M, lanes, 0, [&] { on_scan_scored_body(c, a, o, sa); });
    else kw::launch(grid < M ? grid : M, lanes, 0, [&] { on_scan_body(c, a, o); });
    std::memcpy(out, lists.data(), (size_t)M * k * sizeof(kai_node_answer));
    std::memcpy(n_out, lens.data(), (size_t)M * 4);
    return KAI_OK;
}

// kai_ops_apply on the session (sim_ops_apply of sim_session.hpp), the operations in the caller's node indices
int kai_tssim_apply(void* h, const kai_op* ops, int n) {
    if (!h || n < 0) return KAI_ERR_INVALID_ARG;
    TsSession& t = *static_cast<TsSession*>(h);
    kai_apply_result res{};
    return sim_ops_apply(t.ss, t.apply, ops, n, 0, 256, res);
}

// the pod read-back and the operations the session's actions committed so far
int kai_tssim_state(void* h, int32_t* pod_status_out, int32_t* pod_node_out, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops) {
    if (!h) return KAI_ERR_INVALID_ARG;
    SimSession& ss = static_cast<TsSession*>(h)->ss;
    if (int rc = ss.finish()) return rc;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops)) return rc;
    ss.pod_state(pod_status_out, pod_node_out);
    return KAI_OK;
}

}  // extern "C"

#ifdef KAI_TSSIM_MAIN
// One fixed case: 2 zones x 3 racks x 4 nodes of 8 GPUs (name ranks the reverse of the indices), two nodes without labels; running pods fill the racks unevenly; pending gangs
// whose root groups require the zone and prefer the rack, prefer the zone, prefer a level the topology does not have, require a level it does not have and prefer the rack,
// or name no preferred level.  Both paths with 256, 100 and 1 lanes and small and large grids: the same score rows and deciles, byte for byte; everything kai_subset_nodes
// returns unchanged; the session as it was; each row a permutation of the deciles calculateNodeScores hands n domains.  Then scored lists over the zone rows: every listed
// node has a score, the deciles do not increase along a list, a NONE row and scores = -1 give kai_ordered_nodes' list, an EMPTY row gives none.
int main() {
    const int Z = 2, RK = 3, PER = 4, N = Z * RK * PER + 2, NJ = 15, RUN = 5, J = NJ + RUN, R = 4, Q = 1, D = Z + Z * RK;
    std::vector<int32_t> jnp(J), jfp(J), jq(J, 0), jprio(J), jpre(J, 1), jfps(J), jnps(J, 1); std::vector<int64_t> jcreated(J); std::vector<uint32_t> juid(J);
    int P = 0;
    for (int j = 0; j < J; j++) { jnp[j] = j < NJ ? 1 + j % 5 : 3; jfp[j] = P; P += jnp[j]; jprio[j] = 50 + j % 2; jfps[j] = j; juid[j] = (uint32_t)j; jcreated[j] = 1000 + j; }
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
        req[0 * P + p] = 1000; req[1 * P + p] = 4000; req[2 * P + p] = running ? 3 : 1 + j % 2; req[3 * P + p] = 1;
    }
    std::vector<int32_t> topo_off = {0, 2}, ndom((size_t)2 * N, -1), dpar(D), dlvl(D); std::vector<uint32_t> drank(D);
    for (int n = 0; n < Z * RK * PER; n++) { const int z = n / (RK * PER), rk = n / PER; ndom[0 * N + n] = z; ndom[1 * N + n] = Z + rk; }
    for (int d = 0; d < D; d++) { dpar[d] = d < Z ? -1 : (d - Z) / RK; dlvl[d] = d < Z ? 0 : 1; drank[d] = (uint32_t)(D - 1 - d); }
    std::vector<int32_t> gjob(J), gpar(J, -1), gtopo(J, 0), greq(J), gpref(J), jroot(J), sgrp(S), stopo(S, -1), sreq(S, -1), spref(S, -1); std::vector<uint32_t> grank(J, 0u);
    for (int j = 0; j < J; j++) {
        gjob[j] = j; jroot[j] = j; sgrp[j] = j; if (j >= NJ) gtopo[j] = -1;
        switch (j % 5) { case 0: greq[j] = 0; gpref[j] = 1; break; case 1: greq[j] = -1; gpref[j] = 0; break; case 2: greq[j] = 0; gpref[j] = 4; break; case 3: greq[j] = 5; gpref[j] = 1; break; default: greq[j] = 0; gpref[j] = -1; }
    }
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
    for (int n = 0; n < N; n++) { if (n < RK * PER) rows[0 * W + (n >> 5)] |= 1u << (n & 31); else rows[1 * W + (n >> 5)] |= 1u << (n & 31); }  // zone 0; zone 1 and the unlabelled nodes
    std::vector<kai_subset_query> qs;
    for (int j = 0; j < J; j++) for (int row = -1; row < NS; row++) { kai_subset_query q; q.job = j; q.group = row == 0 ? j : -1; q.podset = -1; q.nodeset = row; qs.push_back(q); }
    const int M = (int)qs.size(); const int64_t CAP = (int64_t)M * (D + 2);

    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what) { checks++; if (!ok) { bad++; std::printf("FAILED: %s\n", what); } };
    int rc = 0; void* h = kai_tssim_open(&cfg, &s, 1, &rc);
    if (!h) { std::printf("open failed: %d\n", rc); return 2; }
    struct Out { int status = 99, same = 0; kai_subset_result res{}; std::vector<kai_subset_answer> ans; std::vector<kai_node_set> sets; std::vector<uint32_t> maps; int64_t n = -3; std::vector<kai_topo_score_row> sr; std::vector<uint8_t> dec; };
    auto run = [&](int scored, uint32_t flags, int lanes, int wgs, Out& o) {
        kai_subset_answer pa; std::memset(&pa, 0x77, sizeof pa); kai_node_set pz; std::memset(&pz, 0x77, sizeof pz); kai_topo_score_row pr; std::memset(&pr, 0x77, sizeof pr);
        o.ans.assign((size_t)M, pa); o.sets.assign((size_t)CAP, pz); o.maps.assign((size_t)CAP * W, 0x77777777u); o.sr.assign((size_t)M, pr); o.dec.assign((size_t)M * D, 0x77);
        o.status = kai_tssim_subset(h, scored, flags, lanes, wgs, qs.data(), M, rows.data(), NS, o.ans.data(), o.sets.data(), CAP, &o.n, o.maps.data(), o.sr.data(), o.dec.data(), &o.res, &o.same);
    };
    auto same_sets = [&](const Out& x, const Out& y) {
        return x.n == y.n && std::memcmp(x.ans.data(), y.ans.data(), (size_t)M * sizeof(kai_subset_answer)) == 0 && std::memcmp(x.sets.data(), y.sets.data(), (size_t)x.n * sizeof(kai_node_set)) == 0 &&
               std::memcmp(x.maps.data(), y.maps.data(), (size_t)x.n * W * 4) == 0;
    };
    auto same_scores = [&](const Out& x, const Out& y) { return std::memcmp(x.sr.data(), y.sr.data(), (size_t)M * sizeof(kai_topo_score_row)) == 0 && x.dec == y.dec; };
    Out plain; run(0, 0, 256, 1 << 20, plain);
    expect(plain.status == KAI_OK && plain.res.path == KAI_SUBSET_PATH_WIDE && plain.sr[0].level_row == 0x77777777 && plain.dec[0] == 0x77, "kai_subset_nodes writes no scores");
    Out first; bool have = false;
    for (int lanes : {256, 100, 1}) for (int wgs : {3, 1 << 20}) {
        if (lanes == 1 && wgs == 3) continue;
        Out w, e; run(1, 0, lanes, wgs, w); run(1, KAI_SUBSET_ENGINE_PATH, lanes, wgs, e);
        expect(w.status == KAI_OK && w.res.path == KAI_SUBSET_PATH_WIDE && e.status == KAI_OK && e.res.path == KAI_SUBSET_PATH_ENGINE, "the scored call on both paths");
        expect(same_sets(w, plain) && same_sets(e, plain), "everything kai_subset_nodes returns is unchanged");
        expect(same_scores(w, e), "the two paths give the same score rows and deciles");
        expect(w.same && e.same, "the call changes nothing");
        if (!have) { first = w; have = true; } else expect(same_scores(w, first), "every workgroup size and grid: the same scores");
    }
    int kinds[4] = {0, 0, 0, 0}; bool rows_ok = true, bad_level_scored = false;
    for (int i = 0; i < M; i++) {
        const kai_topo_score_row r = first.sr[(size_t)i]; const uint8_t* dr = &first.dec[(size_t)i * D];
        std::vector<int> seen;
        for (int d = 0; d < D; d++) if (dr[d] != KAI_TOPO_NO_SCORE) seen.push_back(dr[d]);
        if (r.level_row < 0) { rows_ok = rows_ok && seen.empty() && r.n_scored == 0; kinds[r.level_row == KAI_TOPO_SCORES_NONE ? 0 : 1]++; continue; }
        kinds[2]++;
        if (first.ans[(size_t)i].status == KAI_SUBSET_BAD_LEVEL) bad_level_scored = true;
        std::sort(seen.begin(), seen.end());
        rows_ok = rows_ok && (int)seen.size() == r.n_scored && r.n_scored > 0 && r.level_row < 2;
        for (int x = 0; x < (int)seen.size() && rows_ok; x++) rows_ok = seen[(size_t)x] == (int)(((double)(x + 1) / (double)r.n_scored) * 10);
        for (int d = 0; d < D && rows_ok; d++) if (dr[d] != KAI_TOPO_NO_SCORE) rows_ok = dlvl[d] == r.level_row;
        if (r.n_scored > 1) kinds[3]++;
    }
    expect(rows_ok, "a row holds the deciles of n_scored domains of the row's level, NONE and EMPTY rows hold none");
    expect(kinds[0] > 0 && kinds[1] > 0 && kinds[2] > 0 && kinds[3] > 0, "NONE, EMPTY, scored rows and rows of several domains all occur");
    expect(bad_level_scored, "a query that ends BAD_LEVEL because of its required level has scores");

    // scored lists: a pod of every pending job over its zone rows, with the job's root row of the call above
    std::vector<kai_scored_query> oq; std::vector<int> row_of;
    for (int j = 0; j < NJ; j++) for (int z = 0; z < NS; z++) { kai_scored_query q; q.pod = jfp[j]; q.nodeset = z; q.flags = 0; q.scores = j * 3; oq.push_back(q); }
    const int OM = (int)oq.size();
    auto lists = [&](int scored, const std::vector<kai_scored_query>& q, int k, int lanes, int grid, std::vector<kai_node_answer>& out, std::vector<int32_t>& len) {
        out.assign((size_t)OM * k, kai_node_answer{-9, -9}); len.assign((size_t)OM, -9);
        return kai_tssim_ordered(h, scored, q.data(), OM, rows.data(), NS, first.sr.data(), first.dec.data(), M, k, lanes, grid, out.data(), len.data());
    };
    std::vector<kai_scored_query> plain_q = oq; for (auto& q : plain_q) q.scores = 0;  // (the pad of a kai_node_query)
    std::vector<kai_scored_query> none_q = oq; for (auto& q : none_q) q.scores = -1;
    for (int k : {1, 8, 64}) for (int lanes : {256, 64}) {
        std::vector<kai_node_answer> u, sc, nn; std::vector<int32_t> ul, sl, nl;
        expect(lists(0, plain_q, k, lanes, 5, u, ul) == 0 && lists(1, oq, k, lanes, 5, sc, sl) == 0 && lists(1, none_q, k, lanes, 5, nn, nl) == 0, "the lists run");
        expect(std::memcmp(u.data(), nn.data(), u.size() * sizeof(kai_node_answer)) == 0 && ul == nl, "scores = -1 gives kai_ordered_nodes' lists");
        bool ok = true; int dropped = 0, reordered = 0;
        for (int i = 0; i < OM && ok; i++) {
            const kai_topo_score_row r = first.sr[(size_t)oq[(size_t)i].scores]; const uint8_t* dr = &first.dec[(size_t)oq[(size_t)i].scores * D];
            if (r.level_row == KAI_TOPO_SCORES_EMPTY) { ok = sl[(size_t)i] == 0; continue; }
            if (r.level_row == KAI_TOPO_SCORES_NONE) { ok = sl[(size_t)i] == ul[(size_t)i] && std::memcmp(&sc[(size_t)i * k], &u[(size_t)i * k], (size_t)k * sizeof(kai_node_answer)) == 0; continue; }
            int last = 11;
            for (int x = 0; x < sl[(size_t)i] && ok; x++) {
                const int n = sc[(size_t)i * k + x].node, dd = ndom[(size_t)r.level_row * N + n];
                ok = dd >= 0 && dr[dd] != KAI_TOPO_NO_SCORE && dr[dd] <= last; if (ok) last = dr[dd];
            }
            if (sl[(size_t)i] < ul[(size_t)i]) dropped++;
            if (sl[(size_t)i] && sc[(size_t)i * k].node != u[(size_t)i * k].node) reordered++;
        }
        expect(ok, "a scored list holds scored nodes only, by non-increasing decile; EMPTY gives none; NONE gives kai_ordered_nodes' list");
        if (k == 64) expect(dropped > 0, "nodes without a score are dropped from a list");
        expect(reordered > 0, "the scores change the head of some list");
    }
    kai_tssim_close(h);
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "topo_scores_sim: %d of %d checks FAILED\n" : "topo_scores_sim: ok (%d checks)\n", bad ? bad : checks, checks);
    return bad ? 1 : 0;
}
#endif
