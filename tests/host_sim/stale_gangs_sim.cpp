// stale_gangs_sim.cpp — TEST INFRASTRUCTURE: kai_stale_gang_eviction's kernel bodies and control flow (kai-scheduler_amd/csrc/kai_stale_gangs.hpp: sg_drive, and through it the
// library's own oa_drive) compiled with plain g++ and run with the emulated lanes of kai_simt.hpp on a session of the host simulation (sim_session.hpp: struct SimSession, opened
// and driven as kai_hostsim_run drives one).  tests/test_stale_gangs.py compares the decision with a numpy restatement of the reference's rules and the state with a TWIN session
// that takes the same operations through kai_ops_apply's emulated apply (mode 1 below: sim_session.hpp sim_ops_apply).  NOT a CPU fallback: libkai_core never contains it; the
// parity claim is tests/test_gpu_stale_gangs.py on the MI355X.
//
// The harness: open the session; run the actions `pre`; make the call on its context; copy the state right behind the call; run the actions `post`; read back.
//
// -DKAI_SGSIM_MAIN adds a main() with one fixed case (the stand-alone program the sanitizers are run on).
#include "sim_session.hpp"
#include "../../kai-scheduler_amd/csrc/kai_stale_gangs.hpp"

namespace {

// the handle's scratch of both entry points: zero between calls
struct Scratch : ApplyScratch {
    std::vector<int32_t> succ, first, wg_e, wg_f; std::vector<int64_t> since; std::vector<uint8_t> expired; std::vector<kai_op> ops; OaHead oa_head{}; SgHead head{};
    void fit(const KaiCtx& c) { ApplyScratch::fit(c.P); if ((int)succ.size() < c.J) succ.assign((size_t)c.J, 0); }
    bool clean(const KaiCtx& c) const { if (!ApplyScratch::clean(c.P)) return false; for (int j = 0; j < c.J; j++) if (succ[j]) return false; return true; }
};
struct SgLauncher : ApplyLauncher {
    Scratch& s;
    explicit SgLauncher(Scratch& sc) : s(sc) {}
    void succeeded(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_succeeded_body(c, a); }); }
    void jobs(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_jobs_body(c, a); }); }
    void first(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_first_body(c, a); }); }
    void totals(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_totals_body(c, a); }); }
    void scan(int b, const SgArgs& a) { kw::launch(1, b, 0, [&] { sg_scan_body(a); }); }
    void emit(int g, int b, const KaiCtx& c, const SgArgs& a) { kw::launch(g, b, 0, [&] { sg_emit_body(c, a); }); }
    int read_counts(SgHead& hd, const SgArgs& a) { hd = *a.head; return 0; }
    int reserve_ops(int n, SgArgs& a, OaArgs& oa) {
        s.ops.assign((size_t)n, kai_op{}); std::memset(&s.oa_head, 0xff, sizeof s.oa_head);  // (k_sg_emit writes the verdict's start values itself)
        a.oa_head = &s.oa_head; a.ops = s.ops.data();
        oa.ops = s.ops.data(); oa.head = &s.oa_head; s.bind(oa);
        return 0;
    }
};

// kai_stale_gang_eviction from its first device call on (the refusals in front of it are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp):
// since [J] in/out, stale_out [J] or NULL, ops_out [cap] (caller's node indices), *n_out; -> what the entry point would return
int sim_stale_gangs(SimSession& ss, Scratch& s, int64_t* since, uint8_t* stale_out, int64_t grace_ns, uint32_t flags, int lanes, int64_t cap, kai_op* ops_out, int64_t* n_out, kai_stale_result& res) {
    KaiCtx& c = ss.ctx(); s.fit(c);
    const int n_wgs = (int)(((int64_t)c.P + lanes - 1) / lanes);
    s.since.assign(since, since + c.J); s.expired.assign((size_t)c.J, 0xee); s.first.assign((size_t)c.J, -7); s.wg_e.assign((size_t)n_wgs + 1, -7); s.wg_f.assign((size_t)n_wgs + 1, -7);
    s.head = SgHead{};
    SgArgs a{}; a.now_ns = c.now_ns; a.grace_ns = grace_ns; a.n_wgs = n_wgs;
    a.head = &s.head; a.since = s.since.data(); a.expired = s.expired.data(); a.succ = s.succ.data(); a.first = s.first.data(); a.wg_e = s.wg_e.data(); a.wg_f = s.wg_f.data();
    SgLauncher l{s}; SgHead hd{}; OaHead hv{}; int path = 0;
    const bool dry = (flags & KAI_STALE_DRY_RUN) != 0;
    int status = sg_drive(l, c, a, lanes, dry, cap, hd, hv, path);
    if (!s.clean(c)) status = KAI_ERR_DEVICE_FAULT;
    if (status == KAI_ERR_CAPACITY) *n_out = hd.n_ops;  // the count needed; nothing else is written
    if (status != KAI_OK) return status;
    if (hd.n_ops > 0 && !dry) ss.state_written(true);  // as kai_ops_apply leaves the handle after evictions
    std::memcpy(since, s.since.data(), (size_t)c.J * 8);
    if (stale_out) std::memcpy(stale_out, s.expired.data(), (size_t)c.J);
    for (int i = 0; i < hd.n_ops; i++) { kai_op o = s.ops[(size_t)i]; o.node = ss.caller_node(o.node); ops_out[i] = o; }
    *n_out = hd.n_ops;
    res.stale_jobs = hd.stale_jobs; res.expired_jobs = hd.expired_jobs; res.n_ops = hd.n_ops; res.path = path; res.pad = 0;
    return status;
}

}  // namespace

extern "C" {

// Runs the actions `pre`, then
//   mode 0: kai_stale_gang_eviction at the clock cfg->now_ns with `grace_ns`, `flags` (KAI_STALE_DRY_RUN) and a capacity of `call_cap` operations, in workgroups of `lanes` lanes:
//           since [J] in/out, stale_out [J] or NULL, sg_ops [call_cap] out, *n_sg_ops out, result out;
//   mode 1: kai_ops_apply's emulated apply of sg_ops[0 .. *n_sg_ops) (the twin);
// then the actions `post`.  call_status: what the entry point would return.  mid_* / hidden: the state right behind the call (hidden: sim_session.hpp StateCopy's words, then fast_ok).
// ops_out ...: the operations of ALL actions and the final state, as kai_hostsim_run returns them (no post action: the state behind the call).
int kai_sgsim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* pre, int n_pre, int mode, int64_t* since, uint8_t* stale_out, int64_t grace_ns, uint32_t flags, int lanes,
                  int64_t call_cap, kai_op* sg_ops, int64_t* n_sg_ops, kai_stale_result* result, int* call_status, const int* post, int n_post,
                  int32_t* mid_status, int32_t* mid_node, kai_queue_share* mid_shares, kai_node_state* mid_nodes, int32_t* hidden, int64_t hidden_cap, int64_t* n_hidden,
                  kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out, kai_queue_share* shares_final, kai_node_state* nodes_out) {
    if (!cfg || !s || n_pre < 0 || n_post < 0 || lanes < 1 || lanes > 4096 || s->n_jobs < 1 || !n_sg_ops || (mode != 0 && mode != 1) || (mode == 0 && (!since || call_cap < 0))) return KAI_ERR_INVALID_ARG;
    if (mode == 1) for (int64_t i = 0; i < *n_sg_ops; i++) if (sg_ops[i].node < 0 || sg_ops[i].node >= s->n_nodes || sg_ops[i].pod < 0 || sg_ops[i].pod >= s->n_pods || sg_ops[i].kind < 0 || sg_ops[i].kind > 2) return KAI_ERR_INVALID_ARG;
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_pre + n_post, n_post > 0)) return rc;  // (as it always was: without a post action, `pre` runs on the sequential engine, as in ops_apply_sim.cpp)
    for (int i = 0; i < n_pre; i++) if (int rc = ss.action(pre[i])) return rc;
    static Scratch scratch; scratch.fit(ss.ctx()); int status = KAI_OK; kai_stale_result res{};
    if (mode == 0) { *n_sg_ops = 0; status = sim_stale_gangs(ss, scratch, since, stale_out, grace_ns, flags, lanes, call_cap, sg_ops, n_sg_ops, res); }
    else if (*n_sg_ops > 0) {
        kai_apply_result ar{};
        status = sim_ops_apply(ss, scratch, sg_ops, (int)*n_sg_ops, 0, lanes, ar);
        if (!scratch.clean(ss.ctx())) status = KAI_ERR_DEVICE_FAULT;
        if (status == KAI_OK) { res.path = ar.path; res.n_ops = (int)*n_sg_ops; ss.state_written(true); }  // as kai_stale_gang_eviction leaves the handle after its evictions
    }
    StateCopy mid = ss.snapshot_state(); mid.hidden.push_back(ss.ctx().fast_ok);
    for (int i = 0; i < n_post; i++) if (int rc = ss.action(post[i])) return rc;
    if (int rc = ss.finish()) return rc;
    if (call_status) *call_status = status;
    if (result) *result = res;
    if (int rc = ss.write(mid, mid_status, mid_node, mid_shares, mid_nodes, hidden, hidden_cap, n_hidden)) return rc;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops)) return rc;
    ss.pod_state(pod_status_out, pod_node_out); ss.shares(shares_final); ss.nodes(nodes_out);
    return KAI_OK;
}

}  // extern "C"

#ifdef KAI_SGSIM_MAIN
// One fixed case: 6 nodes of 8 GPUs whose name ranks are the reverse of their indices, 3 queues, 14 jobs of 3 one-GPU pods with minAvailable 3 (job 13: two pod-sets, 2 + 1):
//   jobs 0-5 running; job 1 lost a pod to Failed (stamped long ago: evicted, two evictions); job 2 lost one (stamped just now: inside its grace); job 3 lost one (never
//   stamped: newly stale); job 4 lost one but has a Succeeded pod (not stale, its old stamp is cleared); job 5: one pod Failed, two Releasing (expired, nothing to evict);
//   jobs 6-11 pending; job 12: a Pipelined and a Running pod, one Failed (expired: the engine walk); job 13: stale through its second pod-set only.
// The call with 256, 100 and 1 lanes: the decision checked against the list above, the state against the twin that takes the same operations through the emulated kai_ops_apply,
// also through the allocate action run behind either; a dry run and a call without capacity write nothing.
int main() {
    const int N = 6, Q = 3, J = 14, PJ = 3, P = J * PJ, R = 4, S = J + 1;
    const int64_t SEC = 1000000000ll, NOW = 1000 * SEC, GRACE = 60 * SEC;
    std::vector<double> alloc((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> nflags(N, 0u), nrank(N), pflags(P, 0u), puid(P), juid(J), quid(Q), psrank(S, 0u);
    std::vector<int32_t> ngc(N, -1), ncls(N, 0), pjob(P), pps(P), pst(P), pnode(P), pprio(P, 0), pcls(P, 0), pnom(P, -1), psjob(S), psmin(S, 3), jq(J), jprio(J, 50), jpre(J), jfp(J), jnp(J, PJ), jfps(J), jnps(J, 1), qpar = {-1, 0, 0}, qprio(Q, 0);
    std::vector<int64_t> pcreated(P), jcreated(J), qcreated(Q);
    for (int n = 0; n < N; n++) { nrank[n] = (uint32_t)(N - 1 - n); alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256000; alloc[2 * N + n] = 8; alloc[3 * N + n] = 110; }
    for (int j = 0; j < J; j++) { psjob[j] = j; jq[j] = 1 + j % 2; jpre[j] = j % 3 != 0; jfp[j] = j * PJ; jfps[j] = j; juid[j] = (uint32_t)j; jcreated[j] = 1000 + j; }
    psjob[J] = 13; jnps[13] = 2; psmin[13] = 2; psmin[14] = 1; psrank[14] = 1;
    for (int p = 0; p < P; p++) {
        const int j = p / PJ; pjob[p] = j; pps[p] = j; puid[p] = (uint32_t)p; pcreated[p] = 2000 + p;
        const bool placed = j < 6 || j >= 12;
        pst[p] = placed ? KAI_POD_RUNNING : KAI_POD_PENDING; pnode[p] = placed ? p % N : -1;
        req[0 * P + p] = 1000; req[1 * P + p] = 4000; req[2 * P + p] = 1; req[3 * P + p] = 1;
    }
    auto lose = [&](int p, int st) { pst[p] = st; };
    lose(1 * PJ + 1, KAI_POD_FAILED); lose(2 * PJ + 0, KAI_POD_FAILED); lose(3 * PJ + 2, KAI_POD_FAILED); lose(4 * PJ + 0, KAI_POD_FAILED); lose(4 * PJ + 1, KAI_POD_SUCCEEDED);
    lose(5 * PJ + 0, KAI_POD_FAILED); lose(5 * PJ + 1, KAI_POD_RELEASING); lose(5 * PJ + 2, KAI_POD_RELEASING);
    lose(12 * PJ + 0, KAI_POD_PIPELINED); lose(12 * PJ + 2, KAI_POD_FAILED);
    pps[13 * PJ + 2] = 14; lose(13 * PJ + 2, KAI_POD_FAILED);
    for (int q = 0; q < Q; q++) { quid[q] = (uint32_t)q; qcreated[q] = 10 + q; }
    std::vector<double> qdes = {384000, 192000, 192000, 1536000, 768000, 768000, 48, 24, 24}, qlim(9, -1.0), qoqw(9, 1.0);
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
    kai_config cfg; std::memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = KAI_ABI_VERSION; cfg.k_value = 1.0; cfg.reclaimer_saturation_multiplier = 1.0; cfg.plugins = KAI_PLUGIN_ALL; cfg.max_consolidation_preemptees = 16;
    cfg.allow_consolidating_reclaim = 1; cfg.full_hierarchy_fairness = 1; cfg.min_node_gpu_memory = 100; for (int i = 0; i < 4; i++) cfg.queue_depth[i] = -1;
    cfg.now_ns = NOW;

    std::vector<int64_t> since0(J, 0);
    since0[1] = NOW - GRACE; since0[2] = NOW - GRACE + 1; since0[4] = NOW - 5 * GRACE; since0[5] = NOW - GRACE - 1; since0[12] = 1; since0[13] = NOW - GRACE;
    since0[6] = 77;  // a pending job that carries a stamp: cleared
    struct Out { int rc = 99, status = 99; kai_stale_result res{}; std::vector<int64_t> since; std::vector<uint8_t> stale; std::vector<kai_op> sg, ops; std::vector<int32_t> st, nd, hidden; std::vector<kai_queue_share> sh; std::vector<kai_node_state> ns; };
    const int ALLOC[1] = {KAI_ACTION_ALLOCATE};
    auto run = [&](int mode, const std::vector<kai_op>* batch, uint32_t flags, int lanes, int64_t cap, bool post, Out& o) {
        o.since = since0; o.stale.assign(J, 9); o.sg.assign((size_t)P, kai_op{}); int64_t n_sg = 0;
        if (batch) { o.sg = *batch; n_sg = (int64_t)batch->size(); o.sg.resize((size_t)P); }
        o.st.assign(P, 0); o.nd.assign(P, 0); o.hidden.assign((size_t)4 * P + 4 * S + 8 * J + 8, 0); o.sh.resize(Q); o.ns.resize(N); int64_t nh = 0, nops = 0;
        o.ops.assign((size_t)8 * P + 64, kai_op{});
        o.rc = kai_sgsim_run(&cfg, &s, nullptr, 0, mode, o.since.data(), o.stale.data(), GRACE, flags, lanes, cap, o.sg.data(), &n_sg, &o.res, &o.status, post ? ALLOC : nullptr, post ? 1 : 0,
                             o.st.data(), o.nd.data(), o.sh.data(), o.ns.data(), o.hidden.data(), (int64_t)o.hidden.size(), &nh, o.ops.data(), (int64_t)o.ops.size(), &nops, nullptr, nullptr, nullptr, nullptr);
        o.hidden.resize((size_t)nh); o.ops.resize((size_t)nops); o.sg.resize((size_t)n_sg);
        return o.rc;
    };
    auto same_state = [&](const Out& a, const Out& b) {
        return a.st == b.st && a.nd == b.nd && a.hidden == b.hidden && std::memcmp(a.sh.data(), b.sh.data(), sizeof(kai_queue_share) * Q) == 0 && std::memcmp(a.ns.data(), b.ns.data(), sizeof(kai_node_state) * N) == 0;
    };
    auto same_ops = [](const std::vector<kai_op>& a, const std::vector<kai_op>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(kai_op)) == 0); };
    int bad = 0, checks = 0;
    auto expect = [&](bool ok, const char* what) { checks++; if (!ok) { bad++; std::printf("FAILED: %s\n", what); } };
    const std::vector<kai_op> none;
    Out open; expect(run(1, &none, 0, 256, 0, false, open) == 0 && open.status == 0, "the untouched session");
    std::vector<int64_t> want_since(J, 0); want_since[1] = since0[1]; want_since[2] = since0[2]; want_since[3] = NOW; want_since[5] = since0[5]; want_since[12] = 1; want_since[13] = since0[13];
    std::vector<uint8_t> want_stale(J, 0); want_stale[1] = want_stale[5] = want_stale[12] = want_stale[13] = 1;
    const int want_pod[6] = {3, 5, 36, 37, 39, 40}, want_stmt[6] = {0, 0, 1, 1, 2, 2};
    Out first; bool have = false;
    for (int lanes : {256, 100, 1}) {
        Out o; expect(run(0, nullptr, 0, lanes, P, false, o) == 0 && o.status == KAI_OK, "the call");
        expect(o.since == want_since && o.stale == want_stale, "timestamps and Stale");
        expect(o.res.stale_jobs == 6 && o.res.expired_jobs == 4 && o.res.n_ops == 6 && o.res.path == KAI_APPLY_PATH_ENGINE && o.sg.size() == 6, "the counts, and the engine walk for a Pipelined pod");
        for (size_t i = 0; i < o.sg.size() && i < 6; i++) { const kai_op& e = o.sg[i];
            expect(e.seq == (int64_t)i && e.kind == KAI_OP_EVICT && e.pod == want_pod[i] && e.node == want_pod[i] % N && e.job == want_pod[i] / PJ && e.stmt == want_stmt[i] && e.pad == 0, "an eviction"); }
        expect(o.st[3] == KAI_POD_RELEASING && o.st[4] == KAI_POD_FAILED && o.st[36] == KAI_POD_RELEASING && o.st[6] == KAI_POD_FAILED && o.st[7] == KAI_POD_RUNNING && o.ns[3].releasing[2] == open.ns[3].releasing[2] + 2, "evicted pods are Releasing on their nodes");
        Out twin; expect(run(1, &o.sg, 0, lanes, 0, false, twin) == 0 && twin.status == KAI_OK && twin.res.path == o.res.path, "the twin takes the operations");
        expect(same_state(o, twin), "the call leaves what kai_ops_apply of its operations leaves");
        if (!have) { first = o; have = true; } else expect(same_state(o, first) && same_ops(o.sg, first.sg), "every workgroup size: the same operations and state");
        Out dry; expect(run(0, nullptr, KAI_STALE_DRY_RUN, lanes, P, false, dry) == 0 && dry.status == KAI_OK && same_state(dry, open), "a dry run writes nothing");
        expect(dry.since == want_since && dry.stale == want_stale && same_ops(dry.sg, o.sg) && dry.res.path == o.res.path && dry.res.n_ops == 6, "... and reports the same");
        Out small; expect(run(0, nullptr, 0, lanes, 5, false, small) == 0 && small.status == KAI_ERR_CAPACITY && small.sg.size() == 6 && same_state(small, open) && small.since == since0, "a capacity below the evictions: the count needed, nothing written");
    }
    {   Out a, b; expect(run(0, nullptr, 0, 256, P, true, a) == 0 && a.status == KAI_OK, "allocate behind the call");
        expect(run(1, &first.sg, 0, 256, 0, true, b) == 0 && b.status == KAI_OK, "allocate behind the twin's apply");
        expect(same_ops(a.ops, b.ops) && !a.ops.empty(), "the next allocate commits the same operations"); }
    {   const int64_t keep = since0[12]; since0[12] = NOW - GRACE + 5; since0[13] = 0;  // without the Pipelined pod's job and the two-pod-set job: placed pods only
        Out o; expect(run(0, nullptr, 0, 256, P, false, o) == 0 && o.status == KAI_OK && o.res.n_ops == 2 && o.res.expired_jobs == 2 && o.res.path == KAI_APPLY_PATH_WIDE && o.since[13] == NOW && o.stale[13] == 0, "placed pods only: the chip-wide path");
        Out twin; expect(run(1, &o.sg, 0, 256, 0, false, twin) == 0 && same_state(o, twin), "... and the twin");
        since0[12] = keep; }
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "stale_gangs_sim: %d of %d checks FAILED\n" : "stale_gangs_sim: ok (%d checks)\n", bad ? bad : checks, checks);
    return bad ? 1 : 0;
}
#endif
