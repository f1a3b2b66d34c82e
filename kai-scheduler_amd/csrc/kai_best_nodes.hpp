// kai_best_nodes.hpp — kai_best_nodes: OrderedNodesByTask + FittingNode (framework/session.go:201-264) for MANY tasks against the session's current node
// state, as three chip-wide launches.  Queries change nothing, so M queries are M independent arg-max reductions over the N nodes:
//
//   k_bn_prep   a thread per query: its ScanReq (Engine::fill_req) and the node-independent first predicate (Engine::task_over_capacity,
//               capacity_policy.go:51-61) from the engine's own source, over a backend whose ctx() is the kernel argument; which (node set, placement
//               resource) pre-order range the query needs.  A thread per bitmap word: the caller's node-set rows re-indexed to name-rank order.
//   k_bn_range  NodePreOrderFn of the bin-pack strategy: getMinMaxPerNode (plugins/nodeplacement/pack.go:66-86) per needed pair, one workgroup each —
//               the arithmetic of CMD_MINMAX (kai_kernels.hpp): DBL_MAX / 0, nodes with allocatable 0 skipped, Idle + Releasing, over the whole node set.
//   k_bn_scan   a workgroup per query (grid-stride): lanes stride over the nodes of the query's row with scan_node_score, keep (orderable(score), node);
//               the fold — wave, then LDS over the waves — takes "greater key, or equal key and lower name rank".
//
// The kernels take KaiCtx by value and write none of the action kernel's LDS objects (g_ctx, g_el, g_sh): many workgroups run at once.  Node state was
// written by earlier kernels on the same stream: plain loads.  No atomics, no waiting on another workgroup; every loop is bounded by N or M.
//
// The bodies are written against kai_simt.hpp, so that tests/host_sim/best_nodes_sim.cpp runs them with emulated lanes on a machine without a GPU.
#pragma once
#include "kai_engine.hpp"
#include "kai_simt.hpp"

namespace kai {

constexpr int KAI_BN_WG = 256;          // lanes of a workgroup of the three kernels
constexpr int KAI_BN_MAX_WAVES = 16;
constexpr int KAI_BN_WGS_PER_CU = 4;    // k_bn_scan's grid is capped at this many workgroups per CU (more queries: grid-stride)

// what k_bn_prep leaves per query
struct BnQuery {
    ScanReq q;
    int32_t row;            // row of the re-indexed bitmaps, -1 = all nodes
    int32_t pipeline_only;
    int32_t dead;           // over its queue's capacity: answers -1 without a scan
    int32_t pair;           // the pre-order range it needs (bn_pair), -1 = none
};
KAI_HD int bn_pair(int row, int r_place) { return 2 * (row + 1) + (r_place == KAI_RES_GPU ? 1 : 0); }  // (all nodes, CPU), (all nodes, GPU), (row 0, CPU), ...

struct BnArgs {
    int32_t M, S, W, pad;                      // queries, node-set rows, words per row
    KAI_GP(const kai_node_query) queries;      // [M]
    KAI_GP(const uint32_t) rows_in;            // [S][W] the caller's rows, caller's node indices
    KAI_GP(const int32_t) perm;                // [N] name rank -> caller's node index (kept on the device from the first call of a session on)
    KAI_GP(uint32_t) rows;                     // [S][W] the rows in name-rank order
    KAI_GP(int32_t) need;                      // [2 (S+1)] pair needed (zeroed by the staging upload)
    KAI_GP(double) range;                      // [2 (S+1)][2] min, max of a needed pair
    KAI_GP(BnQuery) prep;                      // [M]
    KAI_GP(kai_node_answer) out;               // [M]
};

// the engine's pure helpers over the kernel's own context: nothing of the action kernel's LDS objects
struct BnBackend {
    static constexpr bool kVictim = false;
    static constexpr bool kBig = false;
    template <class T> KAI_HD static void assume_tree(T*) {}
    const KaiCtx* cref = nullptr; EngineLocal loc;
    KAI_HD void bind(const KaiCtx& c) { cref = &c; }
    KAI_HD const KaiCtx& ctx() const { return *cref; }
    KAI_HD EngineLocal& local() { return loc; }
};

// monotone map f64 -> u64 (larger double => larger key; never 0 for a number)
KAI_HD uint64_t bn_orderable(double d) {
    uint64_t b; __builtin_memcpy(&b, &d, 8);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
KAI_HD bool bn_in_row(KAI_GP(const uint32_t) bits, int n) { return (bits[n >> 5] >> (n & 31)) & 1u; }

// word w of a caller's node-set row in name-rank order: bit b = the caller's bit of node perm[32 w + b] (kai_subset_nodes.hpp re-indexes its parent rows with it too)
KW_BODY uint32_t bn_reindex_word(int N, KAI_GP(const uint32_t) in, KAI_GP(const int32_t) perm, int w) {
    uint32_t word = 0;
    for (int b = 0; b < 32; b++) {
        const int n = w * 32 + b;
        if (n >= N) break;
        const int o = perm[n];
        word |= ((in[o >> 5] >> (o & 31)) & 1u) << b;
    }
    return word;
}

KW_BODY void bn_prep_body(const KaiCtx& c, const BnArgs& a) {
    const int64_t t = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (t < (int64_t)a.S * a.W) {  // one output word
        const int s = (int)(t / a.W), w = (int)(t % a.W);
        a.rows[(size_t)s * a.W + w] = bn_reindex_word(c.N, a.rows_in + (size_t)s * a.W, a.perm, w);
    }
    if (t < a.M) {
        const kai_node_query qi = a.queries[t];
        BnBackend nb; Engine<BnBackend> eng(c, nb);
        BnQuery o;
        eng.fill_req(o.q, qi.pod);
        o.row = qi.nodeset; o.pipeline_only = (qi.flags & KAI_QUERY_PIPELINE_ONLY) ? 1 : 0;
        o.dead = ((c.plugins & KAI_PLUGIN_PREDICATES) && eng.task_over_capacity(qi.pod)) ? 1 : 0;
        o.pair = -1;
        if (!o.dead && (c.plugins & KAI_PLUGIN_NODEPLACEMENT) && o.q.strategy == KAI_BINPACK) {  // NodePreOrderFn (Engine::find_node)
            o.pair = bn_pair(o.row, o.q.r_place);
            a.need[o.pair] = 1;  // (every writer stores the same value)
        }
        a.prep[t] = o;
    }
}

KW_BODY void bn_range_body(const KaiCtx& c, const BnArgs& a) {
    KW_SHARED double part_lo[KAI_BN_MAX_WAVES], part_hi[KAI_BN_MAX_WAVES];
    const int pair = kw::bid();
    if (!a.need[pair]) return;  // the whole workgroup
    const int row = pair / 2 - 1, r = (pair & 1) ? KAI_RES_GPU : KAI_RES_CPU;
    KAI_GP(const uint32_t) bits = a.rows + (size_t)(row < 0 ? 0 : row) * a.W;
    const int tid = kw::tid(), lanes = kw::bdim(), lane = kw::lane(), wave = tid >> 6;
    const int wl = lanes - wave * 64 < 64 ? lanes - wave * 64 : 64;  // lanes of this wave
    double lo = 1.7976931348623157e308, hi = 0;  // math.MaxFloat64, 0 (pack.go:66-68)
    for (int n = tid; n < c.N; n += lanes) {
        if (row >= 0 && !bn_in_row(bits, n)) continue;
        if (c.n_alloc[(size_t)r * c.N + n] == 0) continue;
        const double cur = c.n_idle[(size_t)r * c.N + n] + c.n_rel[(size_t)r * c.N + n];
        if (cur < lo) lo = cur;
        if (cur > hi) hi = cur;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int src = (lane ^ o) < wl ? (lane ^ o) : lane;
        const double x = kw::shfl(lo, src), y = kw::shfl(hi, src);
        if (x < lo) lo = x;
        if (y > hi) hi = y;
    }
    if (lane == 0) { part_lo[wave] = lo; part_hi[wave] = hi; }
    kw::sync();
    if (tid == 0) {
        const int nw = (lanes + 63) / 64;
        for (int w = 1; w < nw; w++) { if (part_lo[w] < lo) lo = part_lo[w]; if (part_hi[w] > hi) hi = part_hi[w]; }
        a.range[2 * (size_t)pair] = lo; a.range[2 * (size_t)pair + 1] = hi;
    }
}

KW_BODY void bn_scan_body(const KaiCtx& c, const BnArgs& a) {
    KW_SHARED uint64_t part_key[KAI_BN_MAX_WAVES]; KW_SHARED int32_t part_node[KAI_BN_MAX_WAVES];
    const int tid = kw::tid(), lanes = kw::bdim(), lane = kw::lane(), wave = tid >> 6;
    for (int i = kw::bid(); i < a.M; i += kw::gdim()) {
        BnQuery pq = a.prep[i];
        if (pq.dead) {  // the same for every lane
            if (tid == 0) { kai_node_answer ans; ans.node = -1; ans.is_pipeline = 0; a.out[i] = ans; }
            continue;
        }
        if (pq.pair >= 0) { pq.q.min_a = a.range[2 * (size_t)pq.pair]; pq.q.max_a = a.range[2 * (size_t)pq.pair + 1]; }
        const ScanReq& q = pq.q;
        KAI_GP(const uint32_t) bits = a.rows + (size_t)(pq.row < 0 ? 0 : pq.row) * a.W;
        int best = -1; uint64_t bk = 0;
        for (int n = tid; n < c.N; n += lanes) {  // ascending: a later node takes over only with a greater key
            if (pq.row >= 0 && !bn_in_row(bits, n)) continue;
            double sc = 0;
            if (!scan_node_score(c, q, n, sc)) continue;
            const uint64_t k = bn_orderable(sc);
            if (best < 0 || k > bk) { best = n; bk = k; }
        }
        // over the wave: the greatest key, then the lowest name rank among the lanes that hold it (0 = no candidate)
        if (best < 0) bk = 0;
        const uint64_t wk = kw::wave_max_u64(bk);
        const uint64_t mine = (best >= 0 && bk == wk) ? (uint64_t)(0x7fffffff - best) + 1 : 0;
        const uint64_t wn = kw::wave_max_u64(mine);
        if (lane == 0) { part_key[wave] = wk; part_node[wave] = wn ? 0x7fffffff - (int32_t)(wn - 1) : -1; }
        kw::sync();
        if (tid == 0) {
            const int nw = (lanes + 63) / 64;
            int node = -1; uint64_t key = 0;
            for (int w = 0; w < nw; w++) {
                const int n = part_node[w]; const uint64_t k = part_key[w];
                if (n < 0) continue;
                if (node < 0 || k > key || (k == key && n < node)) { node = n; key = k; }  // greater key, or equal key and lower name rank
            }
            kai_node_answer ans; ans.node = -1; ans.is_pipeline = 0;
            if (node >= 0) {
                bool allocatable = q.best_effort || fits(c, q.req, node, false);  // NodeInfo.IsTaskAllocatable (Engine::find_node)
#ifdef KAI_SHARED_GPUS
                if (c.shared_on && q.shared) allocatable = q.best_effort || fits_shared(c, q, node, false);
#endif
                ans.node = a.perm[node];
                ans.is_pipeline = (pq.pipeline_only || !allocatable) ? 1 : 0;
            }
            a.out[i] = ans;
        }
        kw::sync();  // the partial results are read before the next query's overwrite them
    }
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(KAI_BN_WG) k_bn_prep(KaiCtx c, BnArgs a) { bn_prep_body(c, a); }
__global__ void __launch_bounds__(KAI_BN_WG) k_bn_range(KaiCtx c, BnArgs a) { bn_range_body(c, a); }
__global__ void __launch_bounds__(KAI_BN_WG) k_bn_scan(KaiCtx c, BnArgs a) { bn_scan_body(c, a); }
#endif

// Where the pieces of one call lie in the handle's scratch (device) and staging (pinned host) buffers, 16-byte aligned.  The permutation comes first, at an offset no call
// moves; [queries | rows_in | need] is what every call sends, in ONE copy (with the permutation in front of it on the first call of a session).  extra_up: bytes a call
// sends on top (kai_ordered_nodes_scored: its score rows and deciles), behind `need` in the same copy.
struct BnLayout {
    size_t perm, queries, rows_in, need, extra, up_end, rows, range, prep, out, end;
    BnLayout(int N, int M, int S, int W, size_t extra_up = 0) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        perm = o; o = al(o + (size_t)(N > 0 ? N : 1) * 4);
        queries = o; o = al(o + (size_t)M * sizeof(kai_node_query));
        rows_in = o; o = al(o + (size_t)S * W * 4 + 4);
        need = o; o = al(o + (size_t)2 * (S + 1) * 4);
        extra = o; o = al(o + extra_up);
        up_end = o;
        rows = o; o = al(o + (size_t)S * W * 4 + 4);
        range = o; o = al(o + (size_t)2 * (S + 1) * 2 * 8);
        prep = o; o = al(o + (size_t)M * sizeof(BnQuery));
        out = o; o = al(o + (size_t)M * sizeof(kai_node_answer));
        end = o;
    }
};

}  // namespace kai
