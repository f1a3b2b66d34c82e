// ordered_nodes_sim.cpp — TEST INFRASTRUCTURE: the kernel bodies of kai_ordered_nodes (k_bn_prep and k_bn_range of kai_best_nodes.hpp, k_on_scan of
// kai-scheduler_amd/csrc/kai_ordered_nodes.hpp) compiled with plain g++ and run with the emulated lanes of kai_simt.hpp, over a KaiCtx whose node and pod arrays the
// caller supplies (already in name-rank order: kai_bnsim_in of best_nodes_sim.cpp, which this file includes — the library holds kai_bnsim_run too, so that a test asks
// both for the same case).  tests/test_ordered_nodes.py compares the lists with the oracle on a machine without a GPU.  NOT a CPU fallback: libkai_core never contains
// it; the parity claim is tests/test_gpu_ordered_nodes.py on the MI355X.
//
// -DKAI_ONSIM_MAIN adds a main() that runs one fixed case against a serial sort over the same per-node functions (the stand-alone program the sanitizers are run on).
#include <algorithm>

#include "best_nodes_sim.cpp"
#include "../../kai-scheduler_amd/csrc/kai_ordered_nodes.hpp"

extern "C" {

// lanes: threads per workgroup, a multiple of 64 up to 256 (256 on the device); grid: workgroups of the scan (fewer than M: the grid-stride loop).  out: [M][k], n_out: [M].  Returns 0.
int kai_onsim_run(const kai_bnsim_in* in, const kai_node_query* queries, int32_t M, const uint32_t* rows_in, int32_t S, int32_t k, int32_t lanes, int32_t grid,
                  kai_node_answer* out, int32_t* n_out) {
    if (!in || M < 0 || S < 0 || k < 1 || k > KAI_ORDERED_MAX_K || lanes < 64 || lanes > 64 * KAI_ON_MAX_WAVES || lanes % 64 || grid < 1) return -1;
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
    std::vector<BnQuery> prep((size_t)M + 1); std::vector<kai_node_answer> unused((size_t)M + 1);
    const kai_node_answer poison = {-7, -7};  // every entry and every length must be written by the kernel
    std::vector<kai_node_answer> lists((size_t)M * k + 1, poison); std::vector<int32_t> lens((size_t)M + 1, -7);
    BnArgs a; std::memset((void*)&a, 0, sizeof a);
    a.M = M; a.S = S; a.W = W; a.queries = queries; a.rows_in = rows_in; a.perm = in->perm;
    a.rows = rows.data(); a.need = need.data(); a.range = range.data(); a.prep = prep.data(); a.out = unused.data();
    OnArgs o; std::memset((void*)&o, 0, sizeof o);
    o.k = k; o.out = lists.data(); o.n_out = lens.data();
    if (M == 0) return 0;
    const size_t items = (size_t)M > (size_t)S * W ? (size_t)M : (size_t)S * W;
    kw::launch((int)((items + lanes - 1) / lanes), lanes, 0, [&] { bn_prep_body(c, a); });
    if ((c.plugins & KAI_PLUGIN_NODEPLACEMENT) && (c.gpu_strategy == KAI_BINPACK || c.cpu_strategy == KAI_BINPACK)) kw::launch(2 * (S + 1), lanes, 0, [&] { bn_range_body(c, a); });
    kw::launch(grid < M ? grid : M, lanes, 0, [&] { on_scan_body(c, a, o); });
    std::memcpy(out, lists.data(), (size_t)M * k * sizeof(kai_node_answer));
    std::memcpy(n_out, lens.data(), (size_t)M * 4);
    return 0;
}

}  // extern "C"

#ifdef KAI_ONSIM_MAIN
// One fixed case: 300 nodes whose name ranks are the reverse of their indices (more than a workgroup's stride, many ties: few distinct fill levels), 12 pods, three rows;
// both strategies, k = 1, 3, 40 and 64, up to three workgroup shapes, against a serial sort of (score, name rank).
int main() {
    const int N = 300, P = 12, R = 4, W = (N + 31) / 32, S = 3;
    uint64_t rng = 54321; auto next = [&] { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33); };
    std::vector<double> alloc((size_t)R * N), idle((size_t)R * N), rel((size_t)R * N), req((size_t)R * P);
    std::vector<uint32_t> flags(N, 0u); std::vector<int32_t> gcount(N, -1), ncls(N, 0), pcls(P, 0), pnom(P, -1), pjob(P, 0), perm(N);
    for (int n = 0; n < N; n++) {
        perm[n] = N - 1 - n;
        const double g = (n % 5 == 0) ? 0 : 8;
        alloc[0 * N + n] = 64000; alloc[1 * N + n] = 256e9; alloc[2 * N + n] = g; alloc[3 * N + n] = 110;
        for (int r = 0; r < R; r++) { const double a = alloc[(size_t)r * N + n]; const double used = r == 2 ? (g ? next() % 9 : 0) : r == 0 ? 8000.0 * (next() % 8) : r == 1 ? 32e9 * (next() % 8) : next() % 20; const double rl = r == 2 && used ? next() % ((int)used + 1) : 0; idle[(size_t)r * N + n] = a - used; rel[(size_t)r * N + n] = rl; }
    }
    for (int p = 0; p < P; p++) { req[0 * P + p] = 1000.0 * (1 + next() % 8); req[1 * P + p] = 1e9 * (1 + next() % 16); req[2 * P + p] = (p % 3 == 0) ? 0 : 1 + next() % 8; req[3 * P + p] = 1; }
    pnom[5] = 17; pnom[6] = 299;
    const uint8_t fit = 1;
    std::vector<uint32_t> rows_in((size_t)S * W, 0u);
    for (int n = 0; n < N; n++) { rows_in[0 * W + (n >> 5)] |= 1u << (n & 31); if (next() % 4 == 0) rows_in[1 * W + (n >> 5)] |= 1u << (n & 31); }  // row 2 stays empty
    std::vector<kai_node_query> qs;
    for (int p = 0; p < P; p++) for (int s = -1; s < S; s++) { kai_node_query q; q.pod = p; q.nodeset = s; q.flags = (p + s) % 3 == 0 ? KAI_QUERY_PIPELINE_ONLY : 0; q.pad = 0; qs.push_back(q); }
    const int M = (int)qs.size();
    int bad = 0, checked = 0;
    for (int strat = 0; strat < 2; strat++) {
        kai_bnsim_in in; std::memset((void*)&in, 0, sizeof in);
        in.N = N; in.P = P; in.R = R; in.n_pod_classes = 1; in.n_node_classes = 1;
        in.plugins = KAI_PLUGIN_PREDICATES | KAI_PLUGIN_NODEAVAILABILITY | KAI_PLUGIN_RESOURCETYPE | KAI_PLUGIN_NODEPLACEMENT; in.gpu_strategy = strat; in.cpu_strategy = strat;
        in.n_alloc = alloc.data(); in.n_flags = flags.data(); in.n_gpu_count = gcount.data(); in.n_class = ncls.data(); in.n_idle = idle.data(); in.n_rel = rel.data();
        in.p_req = req.data(); in.p_class = pcls.data(); in.p_nominated = pnom.data(); in.p_job = pjob.data(); in.class_fit = &fit; in.perm = perm.data();
        // the serial lists with the SAME fill_req / scan_node_score / fits: they check the rows, the range, the insert, the merge over the waves and the permutation back, not
        // the scoring itself (that is the oracle's part, tests/test_ordered_nodes.py)
        static EngineState st; KaiCtx c; std::memset((void*)&c, 0, sizeof c);
        c.N = N; c.P = P; c.R = R; c.n_pod_classes = 1; c.n_node_classes = 1; c.plugins = in.plugins; c.gpu_strategy = strat; c.cpu_strategy = strat;
        c.n_alloc = alloc.data(); c.n_flags = flags.data(); c.n_gpu_count = gcount.data(); c.n_class = ncls.data(); c.n_idle = idle.data(); c.n_rel = rel.data();
        c.p_req = req.data(); c.p_class = pcls.data(); c.p_nominated = pnom.data(); c.p_job = pjob.data(); c.class_fit = &fit; c.st = &st;
        std::vector<std::vector<kai_node_answer>> want(M);
        for (int i = 0; i < M; i++) {
            BnBackend nb; Engine<BnBackend> eng(c, nb); ScanReq q; eng.fill_req(q, qs[i].pod);
            auto in_set = [&](int n) { const int o = perm[n]; return qs[i].nodeset < 0 || ((rows_in[(size_t)qs[i].nodeset * W + (o >> 5)] >> (o & 31)) & 1u); };
            if (q.strategy == KAI_BINPACK) {
                double lo = 1.7976931348623157e308, hi = 0;
                for (int n = 0; n < N; n++) { if (!in_set(n) || alloc[(size_t)q.r_place * N + n] == 0) continue; const double cur = idle[(size_t)q.r_place * N + n] + rel[(size_t)q.r_place * N + n]; if (cur < lo) lo = cur; if (cur > hi) hi = cur; }
                q.min_a = lo; q.max_a = hi;
            }
            std::vector<std::pair<double, int>> cand;
            for (int n = 0; n < N; n++) { double sc = 0; if (in_set(n) && scan_node_score(c, q, n, sc)) cand.push_back({sc, n}); }
            std::stable_sort(cand.begin(), cand.end(), [](const std::pair<double, int>& x, const std::pair<double, int>& y) { return x.first > y.first; });  // (ascending name rank among equal scores)
            for (const auto& x : cand) { kai_node_answer w; w.node = perm[x.second]; w.is_pipeline = ((qs[i].flags & 1) || !(q.best_effort || fits(c, q.req, x.second, false))) ? 1 : 0; want[i].push_back(w); }
        }
        const int shapes[3][2] = {{256, 7}, {64, M}, {128, 3}};
        for (int k : {1, 3, 40, 64}) for (const auto& sh : shapes) {
            if (k == 40 && sh[0] != 128) continue;  // (the program stays a matter of seconds)
            std::vector<kai_node_answer> got((size_t)M * k); std::vector<int32_t> len(M);
            if (kai_onsim_run(&in, qs.data(), M, rows_in.data(), S, k, sh[0], sh[1], got.data(), len.data())) { std::printf("run failed\n"); return 2; }
            for (int i = 0; i < M; i++) {
                const int n = (int)std::min<size_t>(want[i].size(), (size_t)k);
                bool ok = len[i] == n;
                for (int j = 0; j < k && ok; j++) { const kai_node_answer w = j < n ? want[i][j] : kai_node_answer{-1, 0}; ok = got[(size_t)i * k + j].node == w.node && got[(size_t)i * k + j].is_pipeline == w.is_pipeline; }
                checked++;
                if (!ok && bad++ < 10) std::printf("strategy %d k %d lanes %d grid %d query %d: length %d (want %d), head (%d, %d)\n", strat, k, sh[0], sh[1], i, len[i], n, got[(size_t)i * k].node, got[(size_t)i * k].is_pipeline);
            }
        }
    }
    for (char* s : kw::emu().stacks) std::free(s);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    std::printf(bad ? "ordered_nodes_sim: %d MISMATCHES\n" : "ordered_nodes_sim: ok (%d)\n", bad ? bad : checked);
    return bad ? 1 : 0;
}
#endif
