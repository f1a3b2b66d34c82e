// kai_ordered_nodes.hpp — kai_ordered_nodes: the first K entries of OrderedNodesByTask (framework/session.go:201-264) with the nodes that fail FittingNode dropped, for
// MANY tasks against the session's current node state.  The reference's walk (actions/common/allocate.go) tries the list's nodes one after the other; kai_best_nodes
// answers its head.  Three chip-wide launches: k_bn_prep and k_bn_range of kai_best_nodes.hpp as they are (the same BnArgs: the query's ScanReq, its `dead` flag, the
// rows in name-rank order, the pre-order range ONCE over the whole node set), then
//
//   k_on_scan   a workgroup per query (grid-stride), ONE scoring pass: every wavefront keeps the K best (orderable(score), node) of the nodes it strides over in
//               registers — lane j holds entry j, sorted by "greater key, or equal key and lower name rank"; lanes K .. 63 hold what fell off the end, still in order.
//               A stride scores 64 nodes (scan_node_score, once per node), ballots the lanes whose candidate beats entry K-1, and inserts those one by one: the
//               candidate is broadcast, its position is the number of entries that beat it (popcount of a ballot), the entries from there on move up a lane.  After
//               the first few strides the ballot is almost always empty.  The waves then leave their lists in LDS and wave 0 inserts the other waves' entries by the
//               same routine; its lanes j < K compute is_pipeline for their node as bn_scan_body does for its one, map it through perm and store out[i K + j].
//
// The list is NOT "kai_best_node with the winners removed": under bin-packing NodePreOrderFn scales the pack score with the minimum and maximum of Idle + Releasing over
// the node set it is given (plugins/nodeplacement/pack.go:66-86), so a node set without the winner can order the remaining nodes differently.
//
// As kai_best_nodes.hpp:12: KaiCtx by value, none of the action kernel's LDS objects, plain loads and vector stores, no atomics, no waiting on another workgroup; every
// loop is bounded by N, M or K (a ballot has 64 bits).  Every cross-lane call is reached by whole wavefronts: the stride's trip count and the loop over a ballot's bits
// are the same in every lane of a wavefront, and a lane without a node of its own takes part with an empty candidate.  The block size is a multiple of 64.
//
// kai_ordered_nodes_scored adds the topology plugin's term (nodeOrderFn, plugins/topology/node_scoring.go:17-35) in k_on_scan_scored, the same body with SCORED set: a query
// names a row of score rows / deciles (kai_subset_nodes_scored's outputs, sent with the queries); a node's domain at the row's level is one coalesced load of node_domain per
// stride, its decile a byte gather from the query's row (a few hundred bytes every lane of the workgroup reads: left to the caches).  A node without a score is dropped, the
// others get decile x 10 000 on top — the rule of CMD_BEST (kai_kernels.hpp).  k_on_scan itself is compiled from SCORED = false and carries none of it.
//
// Written against kai_simt.hpp, so that tests/host_sim/ordered_nodes_sim.cpp runs the body with emulated lanes on a machine without a GPU.
#pragma once
#include <cstddef>

#include "kai_best_nodes.hpp"

namespace kai {

constexpr int KAI_ON_MAX_WAVES = KAI_BN_WG / 64;  // wavefronts of a workgroup of k_on_scan
constexpr int32_t KAI_ON_NO_NODE = 0x7fffffff;    // the node of an empty entry (key 0): every real entry beats it
static_assert(KAI_ORDERED_MAX_K == 64, "an entry per lane of a wavefront");

struct OnArgs {
    int32_t k, pad;
    KAI_GP(kai_node_answer) out;  // [M][k]
    KAI_GP(int32_t) n_out;        // [M]
};

// the score rows of a scored call, [n_rows] and [n_rows][D] (D = the snapshot's domains)
struct OnScoreArgs {
    int32_t D, pad;
    KAI_GP(const kai_topo_score_row) rows;
    KAI_GP(const uint8_t) deciles;
};
static_assert(sizeof(kai_scored_query) == sizeof(kai_node_query) && offsetof(kai_scored_query, scores) == offsetof(kai_node_query, pad), "k_bn_prep reads a scored query as a kai_node_query");

// the list's order: greater key, or equal key and lower name rank (nodes are distinct: a strict order; key 0 = an empty entry, last)
KAI_HD bool on_beats(uint64_t ka, int32_t na, uint64_t kb, int32_t nb) { return ka > kb || (ka == kb && na < nb); }

// One stride's worth of candidates (ck, cn; ck 0 = none) into the wavefront's sorted list (ek, en: lane j holds entry j).  The whole wavefront calls it.
KW_BODY void on_insert(uint64_t& ek, int32_t& en, uint64_t ck, int32_t cn, int k) {
    const int lane = kw::lane();
    const uint64_t lk = kw::bcast(ek, k - 1); const int32_t ln = kw::bcast(en, k - 1);
    uint64_t m = kw::ballot(ck != 0 && on_beats(ck, cn, lk, ln));  // the same in every lane: so is the loop over its bits (at most 64)
    while (m) {
        const int src = __builtin_ctzll(m); m &= m - 1;
        const uint64_t bk = kw::bcast(ck, src); const int32_t bn = kw::bcast(cn, src);
        const int pos = __builtin_popcountll(kw::ballot(on_beats(ek, en, bk, bn)));  // the entries that beat it are a prefix of the sorted list (64: it falls off)
        const uint64_t uk = kw::shfl_up(ek, 1); const int32_t un = kw::shfl_up(en, 1);
        if (lane > pos) { ek = uk; en = un; }
        if (lane == pos) { ek = bk; en = bn; }
    }
}

template <bool SCORED>
KW_BODY void on_scan_body_t(const KaiCtx& c, const BnArgs& a, const OnArgs& o, const OnScoreArgs& s) {
    KW_SHARED uint64_t l_key[KAI_ON_MAX_WAVES * 64]; KW_SHARED int32_t l_node[KAI_ON_MAX_WAVES * 64];
    const int tid = kw::tid(), lanes = kw::bdim(), lane = kw::lane(), wave = tid >> 6, nw = lanes >> 6, k = o.k;
    for (int i = kw::bid(); i < a.M; i += kw::gdim()) {
        BnQuery pq = a.prep[i];
        KAI_GP(kai_node_answer) out = o.out + (size_t)i * k;
        int trow = -1; KAI_GP(const uint8_t) dec = nullptr;  // the level row the nodes' domains are read from and the query's deciles; -1: no topology term
        if (SCORED) {
            const int sr = a.queries[i].pad;  // (kai_scored_query.scores)
            if ((c.plugins & KAI_PLUGIN_TOPOLOGY) && sr >= 0) {
                const int lr = s.rows[sr].level_row;
                if (lr == KAI_TOPO_SCORES_EMPTY) pq.dead = 1;  // scores were recorded and no node has one: every node is dropped
                else if (lr >= 0) { trow = lr; dec = s.deciles + (size_t)sr * (size_t)s.D; }
            }
        }
        if (pq.dead) {  // the same for every lane
            if (tid < k) { kai_node_answer ans; ans.node = -1; ans.is_pipeline = 0; out[tid] = ans; }
            if (tid == 0) o.n_out[i] = 0;
            continue;
        }
        if (pq.pair >= 0) { pq.q.min_a = a.range[2 * (size_t)pq.pair]; pq.q.max_a = a.range[2 * (size_t)pq.pair + 1]; }
        const ScanReq& q = pq.q;
        KAI_GP(const uint32_t) bits = a.rows + (size_t)(pq.row < 0 ? 0 : pq.row) * a.W;
        uint64_t ek = 0; int32_t en = KAI_ON_NO_NODE;
        for (int base = wave * 64; base < c.N; base += lanes) {  // the trip count is the wavefront's, not the lane's
            const int n = base + lane;
            double sc = 0;
            bool ok = n < c.N && (pq.row < 0 || bn_in_row(bits, n)) && scan_node_score(c, q, n, sc);
            if (SCORED && trow >= 0 && n < c.N) {  // a node without a score is dropped (framework/session.go:247-251)
                const int dd = c.node_domain[(size_t)trow * c.N + n];
                const int dv = (ok && dd >= 0 && dd < s.D) ? dec[dd] : KAI_TOPO_NO_SCORE;
                if (dv == KAI_TOPO_NO_SCORE) ok = false; else sc += dv * KAI_TOPO_SCORE_UNIT;
            }
            on_insert(ek, en, ok ? bn_orderable(sc) : 0, n, k);
        }
        if (nw > 1) {
            l_key[tid] = ek; l_node[tid] = en;
            kw::sync();
            if (wave == 0) for (int w = 1; w < nw; w++) on_insert(ek, en, l_key[w * 64 + lane], l_node[w * 64 + lane], k);
        }
        if (wave == 0) {
            const bool have = lane < k && ek != 0;
            const uint64_t filled = kw::ballot(have);
            if (lane < k) {
                kai_node_answer ans; ans.node = -1; ans.is_pipeline = 0;
                if (have) {
                    bool allocatable = q.best_effort || fits(c, q.req, en, false);  // NodeInfo.IsTaskAllocatable (Engine::find_node), per node of the list
#ifdef KAI_SHARED_GPUS
                    if (c.shared_on && q.shared) allocatable = q.best_effort || fits_shared(c, q, en, false);
#endif
                    ans.node = a.perm[en];
                    ans.is_pipeline = (pq.pipeline_only || !allocatable) ? 1 : 0;
                }
                out[lane] = ans;
            }
            if (lane == 0) o.n_out[i] = __builtin_popcountll(filled);
        }
        if (nw > 1) kw::sync();  // the lists are read before the next query's overwrite them
    }
}

KW_BODY void on_scan_body(const KaiCtx& c, const BnArgs& a, const OnArgs& o) { on_scan_body_t<false>(c, a, o, OnScoreArgs{}); }
KW_BODY void on_scan_scored_body(const KaiCtx& c, const BnArgs& a, const OnArgs& o, const OnScoreArgs& s) { on_scan_body_t<true>(c, a, o, s); }

#if defined(__HIPCC__)
__global__ void __launch_bounds__(KAI_BN_WG) k_on_scan(KaiCtx c, BnArgs a, OnArgs o) { on_scan_body(c, a, o); }
__global__ void __launch_bounds__(KAI_BN_WG) k_on_scan_scored(KaiCtx c, BnArgs a, OnArgs o, OnScoreArgs s) { on_scan_scored_body(c, a, o, s); }
#endif

// kai_ordered_nodes' scratch: kai_best_nodes' layout (the permutation at the same offset, the same upload) with [the lists | their lengths] behind it, one download
struct OnLayout : BnLayout {
    size_t lists, n_out, on_end;
    OnLayout(int N, int M, int S, int W, int k, size_t extra_up = 0) : BnLayout(N, M, S, W, extra_up) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        lists = end; n_out = lists + (size_t)M * k * sizeof(kai_node_answer);  // (a multiple of 8: the lengths follow without a gap)
        on_end = al(n_out + (size_t)M * 4);
    }
    size_t down_bytes(int M, int k) const { return (size_t)M * k * sizeof(kai_node_answer) + (size_t)M * 4; }
};

}  // namespace kai
