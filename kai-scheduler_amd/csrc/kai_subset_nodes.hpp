// kai_subset_nodes.hpp — kai_subset_nodes: the topology plugin's subSetNodesFn (plugins/topology/job_filtering.go:34-112) for MANY jobs, sub-groups or pod-sets over the
// session's CURRENT state: the node sets the allocate action would walk, in its order, as records and bitmap rows.  Queries change nothing, so M queries are M independent walks.
//
// The common front:
//   k_sn_tta      a thread per query: the job's tasks-to-allocate chunk where its cache is invalid (Engine::ensure_tta, as k_job_init derives it).  A launch of its own: the
//                 chunk one thread writes is read by the threads of the NEXT launch only.
//   k_sn_prep     a thread per query: the sub-group and its constraint, the early exits (no plugin / topology -2 / no constraint / no task), Engine::subset_tasks over the chunk
//                 (count, summed and maximal request, homogeneity, onePodOnly) and whether active pods restrict the sub-trees.  A thread per bitmap word: the parent rows
//                 re-indexed to name-rank order (bn_reindex_word of kai_best_nodes.hpp).
// CHIP-WIDE PATH.  k_sn_wide, a workgroup per live query (grid-stride), on domain tables of the workgroup's own in the handle's scratch:
//   survey        lanes stride over the nodes of the parent row that are part of the topology: per level the smallest and largest domain (LDS atomics), which gives the
//                 common domain with lowestCommonDomainID's stop at the preferred level; then over the nodes of that domain: Idle + Releasing per resource and, for
//                 homogeneous tasks, the pods of the maximal request the node accommodates (Engine's fits with k x the maximal pod by repeated addition) into the node's
//                 leaf domain — atomic adds of amounts that add exactly in any order (the path's condition), so the sums do not depend on scheduling.
//   tree          level by level up to the common domain, inside its sub-tree; checkJobDomainFit on the common domain; getJobRatioToFreeResources per domain
//                 (Engine::job_ratio_fr); a child's place among its siblings = the siblings with (greater ratio, or equal ratio and lower domain_id_rank), down to the
//                 preferred (else required) level — by domain index where sortTreeFromRoot does not come; the path from the root as a number; the fitting domains of the
//                 relevant levels; a chosen domain's place = the chosen ones in front of it (deeper level, or the same level and a smaller path).
// ENGINE PATH.  k_sn_engine: one lane calls Engine::subset_nodes query by query (its serial form: a backend without scan lanes) and copies the sets out.  Every session.
// Both paths leave per query up to `stride` raw records (domain, allocatable pods) and an answer; then
//   k_sn_offsets  one workgroup: the running sum of the counts = every query's `first`, and the total (one small download for the capacity check)
//   k_sn_emit     a workgroup per record (grid-stride): the kai_node_set and its bitmap row in the caller's node indices, a lane per output word; n_nodes = the popcounts.
//
// The chip-wide kernels take KaiCtx by value, read the session only (k_sn_tta apart) and use none of dom_alloc_pods / dom_free / dom_tmp / dom_ratio / dom_key / dom_children:
// the children table they read is the open's, kept with the handle.  No kernel waits on another workgroup; every loop is bounded by N, the domains, a sibling set, the tree's
// depth, a job's pods or a node's pod slots; every cross-lane call (the barriers, the scan of k_sn_offsets) is reached by whole workgroups.
// The bodies are written against kai_simt.hpp: tests/host_sim/subset_nodes_sim.cpp runs them and sn_drive with emulated lanes.
#pragma once
#include <algorithm>

#include "kai_best_nodes.hpp"
#include "kai_open_kernels.hpp"

namespace kai {

constexpr int KAI_SN_WG = 256;            // lanes of a workgroup of every kernel here (the emulator also runs them with 100 and 1)
constexpr int KAI_SN_WGS_PER_CU = 4;      // k_sn_wide's and k_sn_emit's grids are capped at this many workgroups per CU (more items: grid-stride), as k_bn_scan's is
constexpr int KAI_SN_NODE_PODS = 1 << 20; // bound of the accommodation loop beyond anything a node's pod slots allow

struct SnHead { int64_t total; int32_t fault, fault_line, pad[12]; };
static_assert(sizeof(SnHead) == 64, "SnHead is one 64-byte record in front of the call's upload");
struct SnRaw { int32_t domain, alloc_pods; };  // engine's domain index (D + t: the root of topology t; -1: the parent set as it is)
struct SnPrep {
    SubsetTasks sum;
    int32_t topo, req, pref, early;       // early: the answer was decided in k_sn_prep
    int32_t job, grp, ps, restrict_active;
};

struct SnArgs {
    int32_t M, S, W, stride;              // queries, parent rows, words per row, raw records a query can have (domains of the largest topology + 1)
    int32_t want_bitmaps, want_scores, pad1, pad2;  // want_scores (kai_subset_nodes_scored): the preferred-level scores into score_rows / deciles; 0 = not wanted
    KAI_GP(SnHead) head;
    KAI_GP(const kai_subset_query) queries;  // [M]
    KAI_GP(const uint32_t) rows_in;       // [S][W] the caller's rows, caller's node indices
    KAI_GP(const int32_t) perm;           // [N] name rank -> caller's node index   } kept on the device from the
    KAI_GP(const int32_t) rank;           // [N] caller's node index -> name rank   } first call of a session on
    KAI_GP(const int32_t) children;       // [dom_child_off[D + T]] the children table as the open built it (no action re-orders this copy)
    KAI_GP(uint32_t) rows;                // [S][W] the rows in name-rank order
    KAI_GP(SnPrep) prep;                  // [M]
    KAI_GP(kai_subset_answer) answers;    // [M]
    KAI_GP(SnRaw) raw;                    // [M][stride]
    KAI_GP(int32_t) etmp;                 // [stride] engine path: the sets of the running query
    // chip-wide path, [workgroups of k_sn_wide][D + T]: free resources, ratio, path key, allocatable pods, place among the siblings, level if chosen
    KAI_GP(double) w_free; KAI_GP(double) w_ratio; KAI_GP(int64_t) w_key; KAI_GP(int32_t) w_ap; KAI_GP(int32_t) w_place; KAI_GP(int32_t) w_lvl;
    KAI_GP(int32_t) w_sc;                 // ... and, where scores are wanted, 1 for a preferred-level domain of the common domain's sub-tree
    KAI_GP(kai_topo_score_row) score_rows;  // [M]       } what t.subGroupNodeScores[subGroup] holds when the reference's function returns, as deciles (kai_core.h);
    KAI_GP(uint8_t) deciles;              // [M][c.D]  } bound where want_scores is set
    KAI_GP(kai_node_set) sets;            // [total]     } k_sn_emit's outputs, in a buffer of their own
    KAI_GP(uint32_t) bitmaps;             // [total][W]  } (sized once the total is known)
};

// a domain in the caller's encoding
KAI_HD int32_t sn_domain_out(const KaiCtx& c, int d) { return d < 0 ? KAI_SUBSET_PARENT : d >= c.D ? KAI_SUBSET_ROOT(d - c.D) : d; }
KAI_HD void sn_answer(const SnArgs& a, int i, int status, int n_sets, int tasks, int32_t common) {
    kai_subset_answer o; o.status = status; o.n_sets = n_sets; o.first = 0; o.tasks = tasks; o.common_domain = common; o.pad = 0;
    a.answers[i] = o;
}
// calculateNodeScores (node_scoring.go:37-53) without the factor scores.Topology: the reference's arithmetic in double
KAI_HD uint8_t sn_decile(int idx, int n) { const double score = ((double)(idx + 1) / (double)n) * 10; const double t = (double)(int64_t)score; return (uint8_t)(t > score ? t - 1.0 : t); }
KAI_HD void sn_score_row(const SnArgs& a, int i, int level_row, int n_scored) { kai_topo_score_row o; o.level_row = level_row; o.n_scored = n_scored; a.score_rows[i] = o; }
// the sub-group a query names: grp (a SubGroupSet) or ps (a pod-set), and its constraint
struct SnGroup { int32_t grp, ps, topo, req, pref; };
KAI_HD SnGroup sn_group(const KaiCtx& c, const kai_subset_query& q) {
    SnGroup g;
    g.ps = q.podset >= 0 ? q.podset : -1;
    g.grp = g.ps >= 0 ? -1 : (q.group >= 0 ? q.group : c.j_root_group[q.job]);
    g.topo = g.ps >= 0 ? c.s_topo[g.ps] : c.g_topo[g.grp]; g.req = g.ps >= 0 ? c.s_req[g.ps] : c.g_req[g.grp]; g.pref = g.ps >= 0 ? c.s_pref[g.ps] : c.g_pref[g.grp];
    return g;
}

KW_BODY void sn_tta_body(const KaiCtx& c, const SnArgs& a) {
    const int64_t t = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (t >= a.M) return;
    const int j = a.queries[t].job;
    if (c.j_tta_valid[j]) return;
    NullBackend nb; Engine<NullBackend> eng(c, nb);
    eng.ensure_tta(j, true);  // (two queries of one job write the same chunk)
}

KW_BODY void sn_prep_body(const KaiCtx& c, const SnArgs& a) {
    const int64_t t = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (t < (int64_t)a.S * a.W) {
        const int s = (int)(t / a.W), w = (int)(t % a.W);
        a.rows[(size_t)s * a.W + w] = bn_reindex_word(c.N, a.rows_in + (size_t)s * a.W, a.perm, w);
    }
    if (t >= a.M) return;
    const kai_subset_query q = a.queries[t];
    const SnGroup g = sn_group(c, q);
    NullBackend nb; Engine<NullBackend> eng(c, nb);
    const int j = q.job, nt = c.j_tta_n[j];
    const int32_t* chunk = (const int32_t*)(c.tta + c.j_first_pod[j]);
    int tasks = 0;
    for (int i = 0; i < nt; i++) if (eng.task_in_subgroup(chunk[i], g.grp, g.ps)) tasks++;
    SnPrep o;
    eng.subset_tasks(chunk, nt, g.grp, g.ps, tasks, o.sum);
    o.topo = g.topo; o.req = g.req; o.pref = g.pref; o.job = j; o.grp = g.grp; o.ps = g.ps;
    o.restrict_active = eng.subset_restrict_active(j, g.req, g.grp, g.ps) ? 1 : 0;
    // the reference's first decisions (job_filtering.go:38-60)
    int status = KAI_SUBSET_OK, n_sets = -1;
    if (!(c.plugins & KAI_PLUGIN_TOPOLOGY)) n_sets = 1;
    else if (g.topo == -2) { status = KAI_SUBSET_NO_TOPOLOGY; n_sets = 0; }
    else if (g.topo < 0 || tasks == 0) n_sets = 1;
    o.early = n_sets >= 0 ? 1 : 0;
    if (n_sets == 1) { SnRaw r; r.domain = -1; r.alloc_pods = -1; a.raw[(size_t)t * a.stride] = r; }
    a.prep[t] = o;
    if (a.want_scores) sn_score_row(a, (int)t, KAI_TOPO_SCORES_NONE, 0);  // (the walk overwrites it where the function records scores)
    sn_answer(a, (int)t, status, n_sets > 0 ? n_sets : 0, tasks, KAI_SUBSET_PARENT);
}

KW_BODY void sn_wide_body(const KaiCtx& c, const SnArgs& a) {
    KW_SHARED int32_t s_min[KAI_TOPO_SCAN_LEVELS], s_max[KAI_TOPO_SCAN_LEVELS], s_any, s_cnt, s_nsc;
    const int tid = kw::tid(), lanes = kw::bdim(), DT = c.D + c.T, N = c.N, R = c.R;
    NullBackend nb; Engine<NullBackend> eng(c, nb);
    const size_t wb = (size_t)kw::bid() * (size_t)DT;
    KAI_GP(double) fr = a.w_free + wb * KAI_MAX_RES; KAI_GP(double) ratio = a.w_ratio + wb; KAI_GP(int64_t) key = a.w_key + wb;
    KAI_GP(int32_t) ap = a.w_ap + wb; KAI_GP(int32_t) place = a.w_place + wb; KAI_GP(int32_t) lvl = a.w_lvl + wb;
    const bool ws = a.want_scores != 0;
    KAI_GP(int32_t) scd = ws ? a.w_sc + wb : nullptr;
    for (int i = kw::bid(); i < a.M; i += kw::gdim()) {
        const SnPrep pq = a.prep[i];
        KAI_GP(uint8_t) drow = ws ? a.deciles + (size_t)i * (size_t)c.D : nullptr;
        if (ws) for (int d = tid; d < c.D; d += lanes) drow[d] = KAI_TOPO_NO_SCORE;  // (a lane that stores a decile below stores it behind its own 255)
        if (pq.early) continue;  // (the same for every lane)
        const int t = pq.topo, row0 = c.topo_level_off[t], L = c.topo_level_off[t + 1] - row0, root = c.D + t, tasks = pq.sum.tasks, req = pq.req, pref = pq.pref;
        const bool hom = pq.sum.homogeneous != 0;
        KAI_GP(const uint32_t) parent = a.queries[i].nodeset >= 0 ? a.rows + (size_t)a.queries[i].nodeset * a.W : nullptr;
        auto node_dom = [&](int row, int n) { return c.node_domain[(size_t)row * N + n]; };
        // ---- lowestCommonDomainID (common.go:17-67) over the nodes of the parent row that are part of the topology
        if (tid == 0) { s_any = 0; s_cnt = 0; s_nsc = 0; for (int l = 0; l < KAI_TOPO_SCAN_LEVELS; l++) { s_min[l] = 0x7fffffff; s_max[l] = -0x7fffffff - 1; } }
        kw::sync();
        {   int mn[KAI_TOPO_SCAN_LEVELS], mx[KAI_TOPO_SCAN_LEVELS]; bool any = false;
            for (int l = 0; l < KAI_TOPO_SCAN_LEVELS; l++) { mn[l] = 0x7fffffff; mx[l] = -0x7fffffff - 1; }
            if (L > 0) for (int n = tid; n < N; n += lanes) {
                if ((parent && !bn_in_row(parent, n)) || node_dom(row0, n) < 0) continue;
                any = true;
                for (int l = 0; l < L; l++) { const int dd = node_dom(row0 + l, n); if (dd < mn[l]) mn[l] = dd; if (dd > mx[l]) mx[l] = dd; }
            }
            if (any) { kw::atomic_max(&s_any, 1); for (int l = 0; l < L; l++) { kw::atomic_min(&s_min[l], mn[l]); kw::atomic_max(&s_max[l], mx[l]); } }
        }
        kw::sync();
        int domain = root;
        for (int l = 0; l < L; l++) {
            if (!s_any || s_min[l] != s_max[l]) break;
            domain = s_min[l];
            if (pref == l) break;
        }
        if (domain < 0 || domain >= DT) domain = root;  // (node_domain is range-checked by the open)
        const int dl = c.dom_level[domain];
        // ---- treeAllocatableCleanup :438-445; the pod counts of the common domain's sub-tree start at 0 where the tasks are homogeneous
        for (int d = tid; d < DT; d += lanes) {
            if (c.dom_topo[d] != t) continue;
            ap[d] = (hom && eng.dom_in_subtree(d, domain)) ? 0 : -1;
            for (int r = 0; r < KAI_MAX_RES; r++) fr[(size_t)d * KAI_MAX_RES + r] = 0.0;
        }
        kw::sync();
        // ---- calcSubTreeFreeResources :192-211 and calcNodeAccommodation :213-246 per node of the common domain, into its leaf domain
        if (L > 0) for (int n = tid; n < N; n += lanes) {
            if (!(domain == root ? node_dom(row0, n) >= 0 : node_dom(row0 + dl, n) == domain)) continue;
            const int leaf = node_dom(row0 + L - 1, n);
            if (leaf < 0 || leaf >= DT) continue;
            for (int r = 0; r < R; r++) { const double v = c.n_idle[(size_t)r * N + n] + c.n_rel[(size_t)r * N + n]; if (v != 0) kw::atomic_add((double*)&fr[(size_t)leaf * KAI_MAX_RES + r], v); }
            if (!hom) continue;
            int count = 0;
            if (pq.sum.one_pod_only) count = tasks;
            else {
                double cur[KAI_MAX_RES]; for (int r = 0; r < KAI_MAX_RES; r++) cur[r] = pq.sum.mx[r];  // k-th test pod = k x the maximal pod, by repeated addition
                while (count < KAI_SN_NODE_PODS && fits(c, cur, n, true)) { count++; for (int r = 0; r < R; r++) cur[r] += pq.sum.mx[r]; }
            }
            if (count) kw::atomic_add((int32_t*)&ap[leaf], count);
        }
        kw::sync();
        for (int lv = L - 1; lv > dl; lv--) {  // bottom-up inside the sub-tree (the same trip count in every lane)
            for (int d = tid; d < c.D; d += lanes) {
                if (c.dom_topo[d] != t || c.dom_level[d] != lv || !eng.dom_in_subtree(d, domain)) continue;
                const int par = c.dom_parent[d];
                for (int r = 0; r < R; r++) { const double v = fr[(size_t)d * KAI_MAX_RES + r]; if (v != 0) kw::atomic_add((double*)&fr[(size_t)par * KAI_MAX_RES + r], v); }
                if (hom && ap[d]) kw::atomic_add((int32_t*)&ap[par], ap[d]);
            }
            kw::sync();
        }
        // ---- checkJobDomainFit :362-379 on the common domain, then the levels (job_filtering.go:84-100)
        auto dom_fits = [&](int d) { const int p = ap[d]; if (p != -1) return p >= tasks; return !(eng.job_ratio_fr(pq.sum.tr, fr + (size_t)d * KAI_MAX_RES) > 1.0); };
        int status = KAI_SUBSET_OK;
        const bool common_fits = dom_fits(domain);
        if (!common_fits) status = KAI_SUBSET_NO_FIT;
        else if ((req < 0 && pref < 0) || req >= L || pref >= L) status = KAI_SUBSET_BAD_LEVEL;
        // calculateNodeScores (job_filtering.go:87-90) runs behind the common domain's fit and in front of the level checks; rank: the preferred level is one of the topology's
        const bool recorded = ws && common_fits && pref >= 0, rank = recorded && pref < L;
        if (recorded && !rank && tid == 0) sn_score_row(a, i, KAI_TOPO_SCORES_EMPTY, 0);
        const int max_depth = pref >= 0 ? pref : req;
        // sortTreeFromRoot :447-486: every child's place among its siblings (the whole workgroup: two barriers)
        auto sibling_places = [&] {
            for (int d = tid; d < DT; d += lanes) if (c.dom_topo[d] == t) ratio[d] = eng.job_ratio_fr(pq.sum.tr, fr + (size_t)d * KAI_MAX_RES);
            kw::sync();
            for (int d = tid; d < DT; d += lanes) {
                if (c.dom_topo[d] != t) continue;
                if (d >= c.D) { place[d] = 0; continue; }
                const int p = c.dom_parent[d], b0 = c.dom_child_off[p], b1 = c.dom_child_off[p + 1];
                const bool sorted = eng.dom_in_subtree(p, domain) && !(dl <= max_depth && max_depth < c.dom_level[p]);
                const double rx = ratio[d]; const uint32_t ix = c.dom_id_rank[d];
                int r = 0; bool before = true;
                for (int k = b0; k < b1; k++) {
                    const int y = a.children[k];
                    if (y == d) { before = false; continue; }
                    if (sorted) { const double ry = ratio[y]; if (ry > rx || (ry == rx && c.dom_id_rank[y] < ix)) r++; }
                    else if (before) r++;
                }
                place[d] = r;
            }
            kw::sync();
        };
        // every domain's path from the root as a number; where scores are ranked, the preferred-level domains of the common domain's sub-tree and their count (no barrier)
        auto path_keys = [&] {
            int scored = 0;
            for (int d = tid; d < DT; d += lanes) {
                if (rank) scd[d] = 0;
                if (c.dom_topo[d] != t) continue;
                int64_t k = 0, mul = 1;
                for (int x = d, hops = 0; x >= 0 && c.dom_level[x] >= 0 && hops <= KAI_TOPO_SCAN_LEVELS; x = c.dom_parent[x], hops++) { k += (int64_t)place[x] * mul; mul *= DT; }
                key[d] = k;
                if (rank && d < c.D && c.dom_level[d] == pref && eng.dom_in_subtree(d, domain)) { scd[d] = 1; scored++; }
            }
            if (scored) kw::atomic_add(&s_nsc, scored);
        };
        // behind a barrier that follows path_keys: the i-th such domain in tree order (their parents lie above max_depth = pref: sorted sibling sets, so the paths order them
        // as getLevelDomains' depth-first walk does) takes floor((i + 1) / n * 10)
        auto store_deciles = [&] {
            const int n = s_nsc;
            for (int d = tid; d < c.D; d += lanes) {
                if (!scd[d]) continue;
                const int64_t k = key[d];
                int idx = 0;
                for (int e = 0; e < c.D; e++) if (scd[e] && key[e] < k) idx++;
                drow[d] = sn_decile(idx, n);
            }
            if (tid == 0) sn_score_row(a, i, row0 + pref, n);
        };
        if (status != KAI_SUBSET_OK) {  // (every lane read the same tables)
            if (rank) { sibling_places(); path_keys(); kw::sync(); store_deciles(); }  // a bad REQUIRED level: the scores are recorded all the same
            if (tid == 0) sn_answer(a, i, status, 0, tasks, sn_domain_out(c, domain));
            kw::sync();
            continue;
        }
        sibling_places();
        // ---- getJobAllocatableDomains :265-310 over calculateRelevantDomainLevels :381-425, with every domain's path from the root as a number
        path_keys();
        int mask = 0;
        {   bool fp = false, fq = false;
            for (int l = L - 1; l >= -1; l--) { if (l == pref && l >= 0) fp = true; if (l == req && l >= 0) fq = true; if (fp || fq) mask |= 1 << (l + 1); if (fq) break; } }
        int mine = 0;
        for (int d = tid; d < DT; d += lanes) {
            if (c.dom_topo[d] != t) { lvl[d] = -100; continue; }
            const int l = c.dom_level[d];
            bool ch = (mask >> (l + 1)) & 1;
            if (ch && pq.restrict_active) {
                int anc = d;
                for (int hops = 0; anc >= 0 && c.dom_level[anc] > req && hops <= KAI_TOPO_SCAN_LEVELS; hops++) anc = c.dom_parent[anc];
                ch = anc >= 0 && c.dom_level[anc] == req && eng.subset_has_active(pq.job, row0, req, anc, pq.grp, pq.ps);
            }
            if (ch) ch = dom_fits(d);
            lvl[d] = ch ? l : -100;
            if (ch) mine++;
        }
        if (mine) kw::atomic_add(&s_cnt, mine);
        kw::sync();
        const int n_chosen = s_cnt;
        if (rank) store_deciles();
        // ---- sortDomainInfos :526-542: deepest level first, level-order inside a level
        for (int d = tid; d < DT; d += lanes) {
            const int l = lvl[d];
            if (l == -100) continue;
            const int64_t k = key[d];
            int r = 0;
            for (int e = 0; e < DT; e++) { const int le = lvl[e]; if (le == -100) continue; r += (int)((le > l) | ((le == l) & (key[e] < k))); }
            if (r < a.stride) { SnRaw o; o.domain = d; o.alloc_pods = ap[d]; a.raw[(size_t)i * a.stride + r] = o; }
        }
        if (tid == 0) sn_answer(a, i, n_chosen ? KAI_SUBSET_OK : KAI_SUBSET_NO_FIT, n_chosen < a.stride ? n_chosen : a.stride, tasks, sn_domain_out(c, domain));
        kw::sync();  // the tables and the LDS words are read before the next query's overwrite them
    }
}

// The engine walk, by ONE lane (the device: lane 0 of k_sn_engine's only workgroup): Engine::subset_nodes in its serial form, query by query.  The engine's fault word is
// the session's: it leaves as it came.  The slots of the preferred-level scores are the running call's only (n_keys starts at 0 for every query, as for every job of an action).
template <class Backend>
KAI_HD void sn_engine_walk(const KaiCtx& c, Backend& be, const SnArgs& a) {
    Engine<Backend> eng(c, be);
    EngineState& st = *c.st;
    const int fault0 = st.fault, line0 = st.fault_line;
    st.fault = 0; st.fault_line = 0;
    for (int i = 0; i < a.M && !st.fault; i++) {
        const kai_subset_query q = a.queries[i];
        const SnGroup g = sn_group(c, q);
        const int j = q.job;
        const int32_t* chunk = (const int32_t*)(c.tta + c.j_first_pod[j]);
        KAI_GP(const uint32_t) parent = q.nodeset >= 0 ? a.rows + (size_t)q.nodeset * a.W : nullptr;
        be.local().n_keys = 0;
        SubsetWhy why; why.status = KAI_SUBSET_OK; why.tasks = 0; why.common = -1;
        int n = eng.subset_nodes(j, g.ps >= 0 ? -(g.ps + 1) : g.grp, g.topo, g.req, g.pref, g.grp, g.ps, chunk, c.j_tta_n[j], parent, a.etmp, &why);
        if (n > a.stride) n = a.stride;
        for (int k = 0; k < n; k++) { const int d = a.etmp[k]; SnRaw o; o.domain = d; o.alloc_pods = d >= 0 ? c.dom_alloc_pods[d] : -1; a.raw[(size_t)i * a.stride + k] = o; }
        sn_answer(a, i, why.status, n, why.tasks, sn_domain_out(c, why.common));
        if (a.want_scores) {  // slot 0 is the query's (n_keys started at 0): written exactly where the function recorded scores
            KAI_GP(uint8_t) drow = a.deciles + (size_t)i * (size_t)c.D;
            for (int d = 0; d < c.D; d++) drow[d] = KAI_TOPO_NO_SCORE;
            int level_row = KAI_TOPO_SCORES_NONE, n_scored = 0;
            if (be.local().n_keys > 0 && g.topo >= 0) {
                const int L = c.topo_level_off[g.topo + 1] - c.topo_level_off[g.topo];
                if (g.pref >= L) level_row = KAI_TOPO_SCORES_EMPTY;  // (the slot's row lies outside the topology: never handed on)
                else {
                    level_row = c.sg_row[0];
                    KAI_GP(const double) sc = c.sg_score;
                    for (int d = 0; d < c.D; d++) if (sc[d] >= 0) { drow[d] = (uint8_t)(sc[d] / 10000.0); n_scored++; }
                }
            }
            sn_score_row(a, i, level_row, n_scored);
        }
    }
    if (st.fault) { a.head->fault = st.fault; a.head->fault_line = st.fault_line; }
    st.fault = fault0; st.fault_line = line0;
}

// One workgroup: every query's `first` (the running sum of the counts) and the total.  A thread sums a run of consecutive queries, the workgroup scans the threads' sums.
KW_BODY void sn_offsets_body(const KaiCtx&, const SnArgs& a) {
    KW_SHARED int32_t part[64];
    const int tid = kw::tid(), T = kw::bdim(), lane = kw::lane(), wave = tid >> 6;
    const int wl = T - wave * 64 < 64 ? T - wave * 64 : 64;  // lanes of this wave
    const int per = (a.M + T - 1) / T, lo = tid * per < a.M ? tid * per : a.M, hi = lo + per < a.M ? lo + per : a.M;
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += a.answers[i].n_sets;
    const int incl = kw::wave_scan_add(sum);
    if (lane == wl - 1) part[wave] = incl;
    kw::sync();
    int run = incl - sum;
    for (int w = 0; w < wave; w++) run += part[w];
    if (tid == T - 1) a.head->total = (int64_t)run + sum;
    for (int i = lo; i < hi; i++) { a.answers[i].first = run; run += a.answers[i].n_sets; }
}

// A workgroup per record (grid-stride): the kai_node_set and the set's bitmap row in the caller's node indices — the parent row ∩ the domain's nodes (a root: the nodes that are
// part of the topology; -1: the parent row as it is).
KW_BODY void sn_emit_body(const KaiCtx& c, const SnArgs& a) {
    KW_SHARED int32_t s_n;
    const int tid = kw::tid(), lanes = kw::bdim(), N = c.N, W = a.W;
    const int64_t total = a.head->total;
    for (int64_t r = kw::bid(); r < total; r += kw::gdim()) {
        int lo = 0, hi = a.M - 1;  // the record's query: the last one with first <= r (queries without a set share their successor's)
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.answers[mid].first <= r) lo = mid; else hi = mid - 1; }
        const int i = lo, k = (int)(r - a.answers[i].first);
        if (k < 0 || k >= a.stride) continue;  // (the same for every lane)
        const SnRaw raw = a.raw[(size_t)i * a.stride + k];
        const int d = raw.domain, row = a.queries[i].nodeset;
        KAI_GP(const uint32_t) in = a.rows_in + (size_t)(row < 0 ? 0 : row) * W;
        int row0 = 0, dl = -1;
        if (d >= 0) { row0 = c.topo_level_off[c.dom_topo[d]]; dl = c.dom_level[d]; }
        if (tid == 0) s_n = 0;
        kw::sync();
        int cnt = 0;
        for (int w = tid; w < W; w += lanes) {
            uint32_t word = 0;
            for (int b = 0; b < 32; b++) {
                const int o = w * 32 + b;
                if (o >= N) break;
                bool is_in = row < 0 || ((in[w] >> b) & 1u);
                if (is_in && d >= 0) { const int n = a.rank[o]; is_in = dl < 0 ? c.node_domain[(size_t)row0 * N + n] >= 0 : c.node_domain[(size_t)(row0 + dl) * N + n] == d; }
                if (is_in) word |= 1u << b;
            }
            cnt += __builtin_popcount(word);
            if (a.want_bitmaps) a.bitmaps[(size_t)r * W + w] = word;
        }
        if (cnt) kw::atomic_add(&s_n, cnt);
        kw::sync();
        if (tid == 0) { kai_node_set o; o.domain = sn_domain_out(c, d); o.level = d >= 0 ? dl : -1; o.allocatable_pods = raw.alloc_pods; o.n_nodes = s_n; a.sets[r] = o; }
        kw::sync();  // s_n is read before the next record's reset
    }
}

// Where the pieces of one call lie in the handle's scratch (device) and staging (pinned host), 16-byte aligned.  [perm | rank | children] is the session's part, sent with the first
// call of a session; [queries | rows_in | head] is what every call sends, in ONE copy; [head | answers] is what comes back for the count, in one piece.
struct SnLayout {
    size_t perm, rank, children, tab_end, head, answers, count_end, queries, rows_in, up_end, rows, prep, raw, etmp, w_free, w_ratio, w_key, w_ap, w_place, w_lvl, w_sc, score_rows, deciles, end;
    // scored (kai_subset_nodes_scored): [score_rows | deciles of D domains a query] in one piece and the flag table, behind everything kai_subset_nodes has
    SnLayout(int N, int M, int S, int W, int stride, int DT, int n_children, int wgs, bool scored = false, int D = 0) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        perm = o; o = al(o + (size_t)(N > 0 ? N : 1) * 4); rank = o; o = al(o + (size_t)(N > 0 ? N : 1) * 4); children = o; o = al(o + (size_t)(n_children > 0 ? n_children : 1) * 4); tab_end = o;
        queries = o; o = al(o + (size_t)M * sizeof(kai_subset_query)); rows_in = o; o = al(o + (size_t)S * W * 4 + 4); head = o; o += sizeof(SnHead); up_end = o;
        answers = o; o = al(o + (size_t)M * sizeof(kai_subset_answer)); count_end = o;
        rows = o; o = al(o + (size_t)S * W * 4 + 4); prep = o; o = al(o + (size_t)M * sizeof(SnPrep)); raw = o; o = al(o + (size_t)M * stride * sizeof(SnRaw)); etmp = o; o = al(o + (size_t)stride * 4);
        const size_t dw = (size_t)(wgs > 0 ? wgs : 0) * (size_t)(DT > 0 ? DT : 1);
        w_free = o; o = al(o + dw * KAI_MAX_RES * 8); w_ratio = o; o = al(o + dw * 8); w_key = o; o = al(o + dw * 8); w_ap = o; o = al(o + dw * 4); w_place = o; o = al(o + dw * 4); w_lvl = o; o = al(o + dw * 4);
        w_sc = o; o = al(o + (scored ? dw * 4 : 0));
        score_rows = o; o = al(o + (scored ? (size_t)M * sizeof(kai_topo_score_row) : 0)); deciles = o; o = al(o + (scored ? (size_t)M * (size_t)(D > 0 ? D : 0) : 0));
        end = o;
    }
};
inline SnArgs sn_bind_args(unsigned char* d, const SnLayout& L, int M, int S, int W, int stride) {
    SnArgs a{};
    a.M = M; a.S = S; a.W = W; a.stride = stride;
#define SN_B(field) a.field = (decltype(a.field))(d + L.field)
    SN_B(head); SN_B(queries); SN_B(rows_in); SN_B(perm); SN_B(rank); SN_B(children); SN_B(rows); SN_B(prep); SN_B(answers); SN_B(raw); SN_B(etmp);
    SN_B(w_free); SN_B(w_ratio); SN_B(w_key); SN_B(w_ap); SN_B(w_place); SN_B(w_lvl); SN_B(w_sc); SN_B(score_rows); SN_B(deciles);
#undef SN_B
    return a;
}

// What the host can tell before any launch: the chip-wide path needs the topology plugin, quantities that add exactly in any order (the reference sums a domain's nodes in
// Go map order: only then is the sum a function of the set), no shared-GPU requests and no MIG rows (their accommodation counts read per-device tables), and topologies of at
// most KAI_TOPO_SCAN_LEVELS levels whose paths fit 63 bits.  levels_max: the most levels a topology of the session has.
inline bool sn_wide_session(const KaiCtx& c, int levels_max) {
    if (!(c.plugins & KAI_PLUGIN_TOPOLOGY) || !c.exact_sums || c.shared_on || c.mig_on || levels_max > KAI_TOPO_SCAN_LEVELS) return false;
    const int64_t DT = c.D + c.T; int64_t m = 1;
    for (int l = 0; l < levels_max; l++) { if (DT > 0 && m > (int64_t)0x7fffffffffffffffll / DT) return false; m *= DT; }
    return true;
}

// The call's control flow from its first launch to the count, written once against a Launcher (kai_core.hip SnLauncher: HIP launches on the session's stream;
// tests/host_sim/subset_nodes_sim.cpp: the lock-step emulator):  void tta / prep / wide / offsets / emit(grid, lanes, c, a),  int engine(c, a),  int read_head(SnHead&, a)
// (synchronises).  wgs: workgroups of k_sn_wide the scratch has tables for.
template <class L>
int sn_count(L& l, const KaiCtx& c, const SnArgs& a, bool wide, int lanes, int wgs, SnHead& hd, int& path) {
    const int M = a.M;
    l.tta((int)(((int64_t)M + lanes - 1) / lanes), lanes, c, a);
    const int64_t items = std::max<int64_t>(M, (int64_t)a.S * a.W);
    l.prep((int)((items + lanes - 1) / lanes), lanes, c, a);
    if (wide) l.wide(std::max(1, std::min(M, wgs)), lanes, c, a);
    else if (int rc = l.engine(c, a)) return rc;
    l.offsets(1, lanes, c, a);
    if (int rc = l.read_head(hd, a)) return rc;
    if (hd.fault) return KAI_ERR_DEVICE_FAULT;
    path = wide ? KAI_SUBSET_PATH_WIDE : KAI_SUBSET_PATH_ENGINE;
    return KAI_OK;
}

}  // namespace kai

#if defined(__HIPCC__)
namespace kai {
__global__ void __launch_bounds__(KAI_SN_WG) k_sn_tta(KaiCtx c, SnArgs a) { sn_tta_body(c, a); }
__global__ void __launch_bounds__(KAI_SN_WG) k_sn_prep(KaiCtx c, SnArgs a) { sn_prep_body(c, a); }
__global__ void __launch_bounds__(KAI_SN_WG) k_sn_wide(KaiCtx c, SnArgs a) { sn_wide_body(c, a); }
__global__ void __launch_bounds__(KAI_SN_WG) k_sn_offsets(KaiCtx c, SnArgs a) { sn_offsets_body(c, a); }
__global__ void __launch_bounds__(KAI_SN_WG) k_sn_emit(KaiCtx c, SnArgs a) { sn_emit_body(c, a); }
// one wavefront, of which lane 0 walks: the engine without scan lanes (every loop of subset_nodes on the lane itself), over the kernel's own copy of the context
__global__ void __launch_bounds__(64) k_sn_engine(KaiCtx c, SnArgs a) {
    if (threadIdx.x != 0) return;
    NullBackend be;
    sn_engine_walk(c, be, a);
}
}  // namespace kai
#endif
