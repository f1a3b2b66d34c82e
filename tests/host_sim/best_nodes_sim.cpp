// best_nodes_sim.cpp — TEST INFRASTRUCTURE: the three kernel bodies of kai_best_nodes (kai-scheduler_amd/csrc/kai_best_nodes.hpp) compiled with plain g++ and run with
// the emulated lanes of kai_simt.hpp, over a KaiCtx whose node and pod arrays the caller supplies (already in name-rank order).  tests/test_best_nodes.py compares the
// answers with the oracle on a machine without a GPU.  NOT a CPU fallback: libkai_core never contains it; the parity claim is tests/test_gpu_best_nodes.py on the MI355X.
//
// -DKAI_BNSIM_MAIN adds a main() that runs one fixed case against a plain serial loop over the same per-node functions (the stand-alone program the sanitizers are run on).
#define KAI_SHARED_GPUS 1  // as the device library is built (kai_core.hip); the sessions here have no shared GPUs (shared_on = 0)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kai-scheduler_amd/csrc/kai_best_nodes.hpp"

using namespace kai;

extern "C" {

struct kai_bnsim_in {
    int32_t N, P, R, n_pod_classes, n_node_classes;
    uint32_t plugins; int32_t gpu_strategy, cpu_strategy, restrict_nodes, pad;
    const double* n_alloc; const uint32_t* n_flags; const int32_t* n_gpu_count; const int32_t* n_class; const double* n_idle; const double* n_rel;  // [R][N] / [N], name-rank order
    const double* p_req; const int32_t* p_class; const int32_t* p_nominated; const int32_t* p_job;  // [R][P] / [P]; p_nominated in name-rank order
    const uint8_t* class_fit;
    const int32_t* perm;  // [N] name rank -> caller's node index
};

// lanes: threads per workgroup (256 on the device); grid: workgroups of the scan (fewer than M: the grid-stride loop).  Returns 0.
int kai_bnsim_run(const kai_bnsim_in* in, const kai_node_query* queries, int32_t M, const uint32_t* rows_in, int32_t S, int32_t lanes, int32_t grid, kai_node_answer* out) {
    if (!in || M < 0 || S < 0 || lanes < 1 || lanes > 64 * KAI_BN_MAX_WAVES || grid < 1) return -1;
    static EngineState st;  // (static: zeroed; the engine's constructor reads the totals)
    KaiCtx c; std::memset((void*)&c, 0, sizeof c);
    c.N = in->N; c.P = in->P; c.R = in->R; c.n_pod_classes = in->n_pod_classes; c.n_node_classes = in->n_node_classes;
    c.plugins = in->plugins; c.gpu_strategy = in->gpu_strategy; c.cpu_strategy = in->cpu_strategy; c.restrict_nodes = in->restrict_nodes;
    c.n_alloc = in->n_alloc; c.n_flags = const_cast<uint32_t*>(in->n_flags); c.n_gpu_count = in->n_gpu_count; c.n_class = in->n_class;
    c.n_idle = const_cast<double*>(in->n_idle); c.n_rel = const_cast<double*>(in->n_rel);
    c.p_req = in->p_req; c.p_class = in->p_class; c.p_nominated = in->p_nominated; c.p_job = in->p_job;
    c.class_fit = in->class_fit; c.st = &st;
    const int W = (c.N + 31) / 32; c.W = W;
    std::vector<uint32_t> rows((size_t)S * W + 1, 0u); std::vector<int32_t> need((size_t)2 * (S + 1), 0); std::vector<double> range((size_t)4 * (S + 1), 0.0);
    std::vector<BnQuery> prep((size_t)M + 1); std::vector<kai_node_answer> ans((size_t)M + 1);
    BnArgs a; std::memset((void*)&a, 0, sizeof a);
    a.M = M; a.S = S; a.W = W; a.queries = queries; a.rows_in = rows_in; a.perm = in->perm;
    a.rows = rows.data(); a.need = need.data(); a.range = range.data(); a.prep = prep.data(); a.out = ans.data();
    if (M == 0) return 0;
    const size_t items = (size_t)M > (size_t)S * W ? (size_t)M : (size_t)S * W;
    kw::launch((int)((items + lanes - 1) / lanes), lanes, 0, [&] { bn_prep_body(c, a); });
    if ((c.plugins & KAI_PLUGIN_NODEPLACEMENT) && (c.gpu_strategy == KAI_BINPACK || c.cpu_strategy == KAI_BINPACK)) kw::launch(2 * (S + 1), lanes, 0, [&] { bn_range_body(c, a); });
    kw::launch(grid < M ? grid : M, lanes, 0, [&] { bn_scan_body(c, a); });
    std::memcpy(out, ans.data(), (size_t)M * sizeof(kai_node_answer));
    return 0;
}

}  // extern "C"

#ifdef KAI_BNSIM_MAIN
// One fixed case: 70 nodes whose name ranks are the reverse of their indices, 24 pods, three rows; both strategies, 256 lanes and 1 lane, against a serial loop.
int main() {
    const int N = 70, P = 24, R = 4, W = (N + 31) / 32, S = 3;
    uint64_t rng = 12345; auto next = [&] { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33); };
    std::vector<double> alloc((size_t)R * N), idle((size_t)R * N), rel((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> flags(N, 0u); std::vector<int32_t> gcount(N, -1), ncls(N, 0), pcls(P, 0), pnom(P, -1), pjob(P, 0), perm(N);
    for (int n = 0; n < N; n++) {
        perm[n] = N - 1 - n;
        const double g = (n % 5 == 0) ? 0 : 8;
        alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256e9; alloc[2 * N + n] = g; alloc[3 * N + n] = 110;
        for (int r = 0; r < R; r++) { const double a = alloc[(size_t)r * N + n]; const double used = r == 2 ? (g ? next() % 9 : 0) : r == 0 ? 1000.0 * (next() % 60) : r == 1 ? 1e9 * (next() % 200) : next() % 20; const double rl = r == 2 && used ? next() % ((int)used + 1) : 0; idle[(size_t)r * N + n] = a - used; rel[(size_t)r * N + n] = rl; }
    }
    for (int p = 0; p < P; p++) { req[0 * P + p] = 1000.0 * (1 + next() % 8); req[1 * P + p] = 1e9 * (1 + next() % 16); req[2 * P + p] = (p % 3 == 0) ? 0 : 1 + next() % 8; req[3 * P + p] = 1; }
    const uint8_t fit = 1;
    std::vector<uint32_t> rows_in((size_t)S * W, 0u);
    for (int n = 0; n < N; n++) { rows_in[0 * W + (n >> 5)] |= 1u << (n & 31); if (next() % 4 == 0) rows_in[1 * W + (n >> 5)] |= 1u << (n & 31); }  // row 2 stays empty
    std::vector<kai_node_query> qs;
    for (int p = 0; p < P; p++) for (int s = -1; s < S; s++) { kai_node_query q; q.pod = p; q.nodeset = s; q.flags = (p + s) % 3 == 0 ? KAI_QUERY_PIPELINE_ONLY : 0; q.pad = 0; qs.push_back(q); }
    const int M = (int)qs.size();
    int bad = 0;
    for (int strat = 0; strat < 2; strat++) {
        kai_bnsim_in in; std::memset((void*)&in, 0, sizeof in);
        in.N = N; in.P = P; in.R = R; in.n_pod_classes = 1; in.n_node_classes = 1;
        in.plugins = KAI_PLUGIN_PREDICATES | KAI_PLUGIN_NODEAVAILABILITY | KAI_PLUGIN_RESOURCETYPE | KAI_PLUGIN_NODEPLACEMENT; in.gpu_strategy = strat; in.cpu_strategy = strat;
        in.n_alloc = alloc.data(); in.n_flags = flags.data(); in.n_gpu_count = gcount.data(); in.n_class = ncls.data(); in.n_idle = idle.data(); in.n_rel = rel.data();
        in.p_req = req.data(); in.p_class = pcls.data(); in.p_nominated = pnom.data(); in.p_job = pjob.data(); in.class_fit = &fit; in.perm = perm.data();
        std::vector<kai_node_answer> a256(M), a1(M), a70(M);
        if (kai_bnsim_run(&in, qs.data(), M, rows_in.data(), S, 256, 7, a256.data()) || kai_bnsim_run(&in, qs.data(), M, rows_in.data(), S, 1, M, a1.data()) ||
            kai_bnsim_run(&in, qs.data(), M, rows_in.data(), S, 70, 3, a70.data())) { std::printf("run failed\n"); return 2; }
        // a serial walk with the SAME fill_req / scan_node_score / fits: it checks the re-indexed rows, the range, the fold over lanes and waves and the permutation back, not
        // the scoring itself (that is the oracle's part, tests/test_best_nodes.py)
        static EngineState st; KaiCtx c; std::memset((void*)&c, 0, sizeof c);
        c.N = N; c.P = P; c.R = R; c.n_pod_classes = 1; c.n_node_classes = 1; c.plugins = in.plugins; c.gpu_strategy = strat; c.cpu_strategy = strat;
        c.n_alloc = alloc.data(); c.n_flags = flags.data(); c.n_gpu_count = gcount.data(); c.n_class = ncls.data(); c.n_idle = idle.data(); c.n_rel = rel.data();
        c.p_req = req.data(); c.p_class = pcls.data(); c.p_nominated = pnom.data(); c.p_job = pjob.data(); c.class_fit = &fit; c.st = &st;
        for (int i = 0; i < M; i++) {
            BnBackend nb; Engine<BnBackend> eng(c, nb); ScanReq q; eng.fill_req(q, qs[i].pod);
            auto in_set = [&](int n) { const int o = perm[n]; return qs[i].nodeset < 0 || ((rows_in[(size_t)qs[i].nodeset * W + (o >> 5)] >> (o & 31)) & 1u); };
            if (q.strategy == KAI_BINPACK) {
                double lo = 1.7976931348623157e308, hi = 0;
                for (int n = 0; n < N; n++) { if (!in_set(n) || alloc[(size_t)q.r_place * N + n] == 0) continue; const double cur = idle[(size_t)q.r_place * N + n] + rel[(size_t)q.r_place * N + n]; if (cur < lo) lo = cur; if (cur > hi) hi = cur; }
                q.min_a = lo; q.max_a = hi;
            }
            int best = -1; double bs = 0;
            for (int n = 0; n < N; n++) { double sc = 0; if (!in_set(n) || !scan_node_score(c, q, n, sc)) continue; if (best < 0 || sc > bs) { best = n; bs = sc; } }
            kai_node_answer want; want.node = best >= 0 ? perm[best] : -1; want.is_pipeline = best >= 0 ? (((qs[i].flags & 1) || !(q.best_effort || fits(c, q.req, best, false))) ? 1 : 0) : 0;
            for (const kai_node_answer* got : {&a256[i], &a1[i], &a70[i]}) if (got->node != want.node || got->is_pipeline != want.is_pipeline) { if (bad++ < 10) std::printf("strategy %d query %d: got (%d, %d), want (%d, %d)\n", strat, i, got->node, got->is_pipeline, want.node, want.is_pipeline); }
        }
    }
    for (char* s : kw::emu().stacks) std::free(s);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "best_nodes_sim: %d MISMATCHES\n" : "best_nodes_sim: ok (%d)\n", bad ? bad : 2 * M);
    return bad ? 1 : 0;
}
#endif
