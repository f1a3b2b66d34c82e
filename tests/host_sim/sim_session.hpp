// sim_session.hpp — TEST INFRASTRUCTURE: a session of the host simulation as an object.  The engine's control flow (kai::Engine<>, the same header the gfx950 kernel instantiates)
// on a serial node scanner (HostBackend), the batch path's kernels (HostLauncher) and the session-open, action-init and drain kernels (SimOpenLauncher: the library's own launch
// sequences of kai_open_kernels.hpp) on the lock-step emulator, and struct SimSession: open / action / read-backs / snapshot_state.
// host_sim.cpp runs whole cycles on it (kai_hostsim_run); a harness for an entry point that acts on an open session (ops_apply_sim.cpp, stale_gangs_sim.cpp) opens one, runs
// actions, makes its calls on ctx() between them and reads back.  Include it FIRST: the two macros below must stand in front of the engine's headers.  One translation unit per
// library (the switches the kai_hostsim_set_* exports write are statics of this header).  NOT a CPU fallback: libkai_core never contains any of it.
#pragma once
#define KAI_SHARED_GPUS 1  // the host twin carries the shared-GPU engine code (ABI v4), as the device library does (kai_core.hip defines the same)
#include <cstdlib>
static int g_dom_lanes_min = std::getenv("KAI_HOSTSIM_DOM_MIN") ? std::atoi(std::getenv("KAI_HOSTSIM_DOM_MIN")) : 16;  // kai_hostsim_set_dom_lanes_min: tests lower it so that small topologies take the scan-lane forms of the domain loops
#define KAI_DOM_LANES_MIN g_dom_lanes_min
#include <chrono>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../kai-scheduler_amd/csrc/kai_host_prep.hpp"
#include "../../kai-scheduler_amd/csrc/kai_ctx_build.hpp"
#include "../../kai-scheduler_amd/csrc/kai_open_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_driver.hpp"
#include "../../kai-scheduler_amd/csrc/kai_victim_shard.hpp"
#include "../../kai-scheduler_amd/csrc/kai_ops_apply.hpp"
#include "native_bucket_fill.hpp"

using namespace kai;

// the victim search's waves over the ranks of a node-sharded group (kai_victim_shard.hpp): the test's all-gather on host memory, the exchange state of the running action
static int (*g_x_fn)(void*, const void*, void*, int64_t) = nullptr; static void* g_x_user = nullptr; static int g_x_on = 0, g_x_cap = 0; static int64_t g_x_exchanges = 0;
static kai::XShardHost g_xs;
struct HostXIo {  // MultiCtx lives in this process: the "copies" of the device path are plain reads and writes between the wave's two barriers
    kai::MultiCtx* M;
    int pull(int32_t* hdr, int32_t* res, int64_t* cnt, int b, int cap) {
        hdr[0] = M->world; hdr[1] = __atomic_load_n(&M->fault, __ATOMIC_ACQUIRE); hdr[2] = 0; hdr[3] = 0; for (int k = 0; k < 2; k++) { hdr[4 + k] = __atomic_load_n(&M->next[k], __ATOMIC_ACQUIRE); hdr[6 + k] = __atomic_load_n(&M->hit[k], __ATOMIC_ACQUIRE); }
        std::memcpy(res, M->res[b], sizeof(int32_t) * (size_t)cap); std::memcpy(cnt, M->cnt[b], sizeof(int64_t) * kai::KAI_MW_CNT * (size_t)cap); return 0;
    }
    int push(int b, const int32_t* res, const int64_t* cnt, int cap, int hit, int xrun, int fault) {
        std::memcpy(M->res[b], res, sizeof(int32_t) * (size_t)cap); std::memcpy(M->cnt[b], cnt, sizeof(int64_t) * kai::KAI_MW_CNT * (size_t)cap);
        __atomic_store_n(&M->hit[b], hit, __ATOMIC_RELEASE); __atomic_store_n(&M->xrun[b], xrun, __ATOMIC_RELEASE); if (fault) __atomic_store_n(&M->fault, 1, __ATOMIC_RELEASE); return 0;
    }
    int allgather(const void* s, void* r, int64_t n) { return g_x_fn ? g_x_fn(g_x_user, s, r, n) : (int)KAI_ERR_COMM; }
};
namespace {

struct HostBackend {  // serial twin of DevBackend / service_loop (kai_kernels.hpp)
    static constexpr bool kVictim = true;
    template <class T> static void assume_tree(T*) {}
    bool sim_tree(QNode*&, int32_t*&, int32_t*&) { return false; }
    const KaiCtx* cref = nullptr; EngineLocal loc;
    void bind(const KaiCtx& c) { cref = &c; }
    const KaiCtx& ctx() const { return *cref; }
    EngineLocal& local() { return loc; }
    static constexpr bool kBig = true; EngineBig bigv; EngineBig& big() { return bigv; }
    std::vector<uint64_t> s2_key, top_key; std::vector<int32_t> s2_node, top_node;
    static void add_f64(double* p, double v) { *p += v; }
    static void add_i32(int32_t* p, int32_t v) { *p += v; }
    static double coh_f64(const double* p) { return *p; }
    static int32_t coh_i32(const int32_t* p) { return *p; }
    bool topo_scan(const KaiCtx& c, TopoScan& t);  // (below: needs Engine<HostBackend>)
    bool topo_scan_nodes(const KaiCtx& c, TopoScan& t) {  // the node loops of subset_nodes stay serial here; op 4 (build_node_set) word by word as the scan lanes do it
        if (t.op == 15) {  // the survey in a plain loop: what the scan lanes gather (level minima / maxima over `parent`, Idle + Releasing and pod counts per leaf domain)
            const int DT = c.D + c.T;
            t.any = 0; for (int l = 0; l < KAI_TOPO_SCAN_LEVELS; l++) { t.lvl_min[l] = 0x7fffffff; t.lvl_max[l] = -0x7fffffff - 1; }
            for (int n = 0; n < c.N; n++) {
                const int top = c.node_domain[(size_t)t.row0 * c.N + n], leaf = c.node_domain[(size_t)(t.row0 + t.L - 1) * c.N + n];
                if (top < 0 || leaf < 0) continue;
                if (!t.parent || ((t.parent[n >> 5] >> (n & 31)) & 1u)) {
                    t.any = 1;
                    for (int l = 0; l < t.L; l++) { const int dd = c.node_domain[(size_t)(t.row0 + l) * c.N + n]; if (dd < t.lvl_min[l]) t.lvl_min[l] = dd; if (dd > t.lvl_max[l]) t.lvl_max[l] = dd; }
                }
                double av[KAI_MAX_RES];
                for (int r = 0; r < KAI_MAX_RES; r++) av[r] = r < t.R ? c.n_idle[(size_t)r * c.N + n] + c.n_rel[(size_t)r * c.N + n] : 0.0;
                for (int r = 0; r < t.R; r++) c.dom_free[(size_t)leaf * KAI_MAX_RES + r] += av[r];
                if (t.what & 2) c.dom_tmp[2 * DT + leaf] += topo_node_count(t, av);
            }
            return true;
        }
        if (t.op != 4) return false;
        for (int w = 0; w < c.W; w++) {
            uint32_t word = 0; const uint32_t pw = t.parent ? t.parent[w] : 0xffffffffu;
            for (int b = 0; b < 32; b++) {
                const int n = w * 32 + b; if (n >= c.N) break;
                bool in = (pw >> b) & 1u;
                if (in && t.domain >= 0) in = t.dl < 0 ? c.node_domain[(size_t)t.row0 * c.N + n] >= 0 : c.node_domain[(size_t)(t.row0 + t.dl) * c.N + n] == t.domain;
                if (in) word |= 1u << b;
            }
            t.out[w] = word;
        }
        return true;
    }
    bool pfor(const KaiCtx&, const PforReq&) { return false; }
    void or32(uint32_t* w, uint32_t bits) { *w |= bits; }
    void minmax(const KaiCtx& c, int r, double& mn, double& mx) {
        double lo = 1.7976931348623157e308, hi = 0;
        for (int n = 0; n < c.N; n++) {
            if (loc.scope_bits && !((loc.scope_bits[n >> 5] >> (n & 31)) & 1)) continue;
            if (c.n_alloc[(size_t)r * c.N + n] == 0) continue;
            double cur = c.n_idle[(size_t)r * c.N + n] + c.n_rel[(size_t)r * c.N + n];
            if (cur < lo) lo = cur;
            if (cur > hi) hi = cur;
        }
        mn = lo; mx = hi;
    }
    bool eval_nodes(const KaiCtx& c, const ScanReq& q, const int32_t* nodes, int m, double* sc, uint8_t* ok) {  // the single-node re-evaluations of Engine::best_node_kept
        for (int i = 0; i < m; i++) { double s = 0; ok[i] = scan_node_score(c, q, nodes[i], s) ? 1 : 0; sc[i] = s; }
        return true;
    }
    int best_node(const KaiCtx& c, const ScanReq& q, double* score_out = nullptr) {
        int best = -1; double bs = 0;
        for (int n = 0; n < c.N; n++) {
            if (loc.scope_bits && !((loc.scope_bits[n >> 5] >> (n & 31)) & 1)) continue;
            double sc = 0;
            if (!scan_node_score(c, q, n, sc)) continue;
            if (loc.scope_row >= 0) { int dd = c.node_domain[(size_t)loc.scope_row * c.N + n]; double ts = dd >= 0 ? loc.scope_score[dd] : -1.0; if (ts < 0) continue; sc += ts; }
            if (best < 0 || sc > bs) { best = n; bs = sc; }
        }
        if (score_out) *score_out = bs;
        return best;
    }
    void l2(const KaiCtx& c, int k, int sb) {
        uint64_t bk = 0; int bn = 0x7fffffff;
        for (int e = sb * 64; e < std::min(c.NB, sb * 64 + 64); e++) { uint64_t key = c.sum1_key[(size_t)k * c.NB + e]; int n = c.sum1_node[(size_t)k * c.NB + e]; if (key_better(key, n, bk, bn)) { bk = key; bn = n; } }
        s2_key[k * c.NSB + sb] = bk; s2_node[k * c.NSB + sb] = bn;
    }
    void top(const KaiCtx& c, int k) {
        uint64_t bk = 0; int bn = 0x7fffffff;
        for (int sb = 0; sb < c.NSB; sb++) { uint64_t key = s2_key[k * c.NSB + sb]; int n = s2_node[k * c.NSB + sb]; if (key_better(key, n, bk, bn)) { bk = key; bn = n; } }
        top_key[k] = bk; top_node[k] = bn;
    }
    void begin(const KaiCtx& c) {
        if (!c.use_index) return;
        s2_key.assign((size_t)KAI_CMAX * KAI_NSB_MAX, 0); s2_node.assign((size_t)KAI_CMAX * KAI_NSB_MAX, 0); top_key.assign(KAI_CMAX, 0); top_node.assign(KAI_CMAX, 0);
        for (int k = 0; k < c.C; k++) { for (int sb = 0; sb < c.NSB; sb++) l2(c, k, sb); top(c, k); }
    }
    static void build_block(const KaiCtx& c, int k, int b) {
        uint64_t bk = 0; int bn = b * KAI_BLOCK;
        for (int n = b * KAI_BLOCK; n < std::min(c.N, (b + 1) * KAI_BLOCK); n++) { uint64_t key = class_key(c, c.cls[k], n); if (key_better(key, n, bk, bn)) { bk = key; bn = n; } }
        c.sum1_key[(size_t)k * c.NB + b] = bk; c.sum1_node[(size_t)k * c.NB + b] = bn;
    }
    int32_t blocks[KAI_MAXD]; int n = 0;
    bool dirty_add(int b) { for (int i = 0; i < n; i++) if (blocks[i] == b) return true; if (n == KAI_MAXD) return false; blocks[n++] = b; return true; }
    int dirty_count() { return n; }
    void refresh(const KaiCtx& c) {
        for (int i = 0; i < n; i++) for (int k = 0; k < c.C; k++) build_block(c, k, blocks[i]);
        for (int k = 0; k < c.C; k++) { for (int i = 0; i < n; i++) l2(c, k, blocks[i] / 64); top(c, k); }
        n = 0;
    }
    void class_top(const KaiCtx&, int k, uint64_t& key, int& node) { key = top_key[k]; node = top_node[k]; }
    bool all_dead(const KaiCtx& c) { for (int k = 0; k < c.C; k++) if (top_key[k]) return false; return true; }
    // job staging (kai_engine.hpp JobPf): the device hands it to a service wave and overlaps it with the rest of the pop; here it runs in place,
    // with several "lanes" so that the strided pod assignment is exercised
    void stage_async(const KaiCtx& c, int j) {
        if (n) { KAI_JOBPF.job = -1; KAI_JOBPF.ok = 0; return; }
        int bad = 0; for (int lane = 3; lane >= 0; lane--) bad |= stage_job_lane(c, j, KAI_FRAME, KAI_JOBPF, lane, 4);
        KAI_JOBPF.ok = KAI_JOBPF.shape && !bad;
    }
    bool staged(int j) { bool r = KAI_JOBPF.job == j && KAI_JOBPF.ok; KAI_JOBPF.job = -1; return r; }
    void hot(const KaiCtx& c, QNode*& qn, int32_t*& qheap, int32_t*& root_heap) { qn = c.qn; qheap = c.qheap; root_heap = c.root_heap; }
    // several engines of one victim action (MultiCtx): here they are threads of this process
    static void mw_store32(int32_t* p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
    static int32_t mw_load32(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static void mw_store64(int64_t* p, int64_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
    static int64_t mw_load64(const int64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    static int32_t mw_fetch_add32(int32_t* p, int32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_ACQ_REL); }
    static void mw_fetch_min32(int32_t* p, int32_t v) { int32_t o = __atomic_load_n(p, __ATOMIC_ACQUIRE); while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {} }
    static void mw_exchange(const KaiCtx&, MultiCtx* m, int b) { HostXIo io{m}; if (g_xs.wave(io, b)) __atomic_store_n(&m->fault, 1, __ATOMIC_RELEASE); }  // engine 0, between the wave's two barriers
    static void grid_sync(MultiCtx* m, int clear) {
        const int gen = __atomic_load_n(&m->bar_gen, __ATOMIC_ACQUIRE);
        if (__atomic_add_fetch(&m->bar_count, 1, __ATOMIC_ACQ_REL) == m->world) { __atomic_store_n(&m->next[clear], 0, __ATOMIC_RELAXED); __atomic_store_n(&m->hit[clear], 0x7fffffff, __ATOMIC_RELAXED); __atomic_store_n(&m->bar_count, 0, __ATOMIC_RELAXED); __atomic_add_fetch(&m->bar_gen, 1, __ATOMIC_RELEASE); }
        else { long spins = 0; while (__atomic_load_n(&m->bar_gen, __ATOMIC_ACQUIRE) == gen) { if (++spins > 64) std::this_thread::yield(); if (spins > 400000000L) { __atomic_store_n(&m->fault, 1, __ATOMIC_RELEASE); break; } } }
    }
    int64_t clock() {
#if defined(KAI_PROF_VICTIM) && defined(__x86_64__)
        return (int64_t)__builtin_ia32_rdtsc();  // phase clocks of the host-compiled engine (debug builds only)
#else
        return 0;
#endif
    }
};

// TopoScan ops over domains (5..9): the same per-domain bodies the scan lanes of the action kernel run (Engine::topo_dom_body), in a plain loop
bool HostBackend::topo_scan(const KaiCtx& c, TopoScan& t) {
    if (t.op < 5 || t.op == 15) return topo_scan_nodes(c, t);
    HostBackend tmp; Engine<HostBackend> e(c, tmp);
    int cnt = 0;
    for (int d = 0; d < c.D + c.T; d++) cnt += e.topo_dom_body(t, d);
    if (t.op == 9) t.any = cnt;
    return true;
}

static double g_native_fill_ms = 0; static int64_t g_native_fill_launches = 0, g_native_fill_decisions = 0, g_native_fill_diffs = 0;  // the native shadow of the bucket fill, summed since the last read
extern "C" int kai_hostsim_native_fill(double* ms, int64_t* launches, int64_t* decisions, int64_t* diffs) {
    *ms = g_native_fill_ms; *launches = g_native_fill_launches; *decisions = g_native_fill_decisions; *diffs = g_native_fill_diffs;
    g_native_fill_ms = 0; g_native_fill_launches = g_native_fill_decisions = g_native_fill_diffs = 0; return 0;
}
// what the plan kernels were launched with since the last read (tests/test_batch_device_sizes.py asserts the sizes a run reached): the largest workgroup of kb_plan_scan and of
// kb_plan_setup, the longest stream (positions) a kb_plan_scan workgroup and a segmented node took, the most segments a node was cut into, the segments' workgroup
static int64_t g_plan_shapes[6] = {0, 0, 0, 0, 0, 0};
static int64_t plan_longest_stream(const KaiCtx& c, int h) { int64_t m = 0; for (int i = c.bt.h_off[h]; i < c.bt.h_off[h + 1]; i++) m = std::max<int64_t>(m, c.bt.q_cnt[c.bt.h_nodes[i]]); return m; }
extern "C" int kai_hostsim_plan_shapes(int64_t* out) { for (int i = 0; i < 6; i++) { out[i] = g_plan_shapes[i]; g_plan_shapes[i] = 0; } return 0; }
// the batch path's kernels on the lock-step emulator (kai_simt.hpp)
struct HostLauncher {
    void static_rank(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_static_rank(c); }); }
    void static_check(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_static_check(c); }); }
    void qualify(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_qualify(c); }); }
    void nrec(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_build_nrec(c); }); }
    void plan_setup(int g, int b, const KaiCtx& c, RoundParams rp) { g_plan_shapes[1] = std::max<int64_t>(g_plan_shapes[1], b); kw::launch(g, b, 0, [&] { kb_plan_setup(c, rp); }); }
    void plan_leaf(int g, int b, const KaiCtx& c, RoundParams rp) { kw::launch(g, b, 0, [&] { kb_plan_leaf(c, rp); }); }
    void plan_rank(int g, int b, const KaiCtx& c, RoundParams rp) { kw::launch(g, b, 0, [&] { kb_plan_rank(c, rp); }); }
    void plan_gather(int g, int b, const KaiCtx& c, RoundParams rp) { kw::launch(g, b, 0, [&] { kb_plan_gather(c, rp); }); }
    void plan_scan(int g, int b, const KaiCtx& c, RoundParams rp) {
        kw::launch(g, b, 0, [&] { kb_plan_scan(c, rp); });
        g_plan_shapes[0] = std::max<int64_t>(g_plan_shapes[0], b); g_plan_shapes[2] = std::max(g_plan_shapes[2], plan_longest_stream(c, rp.height));  // (q_cnt: as k_plan_setup of this round left it)
    }
    void seg_sum(int g, int b, const KaiCtx& c, RoundParams rp, int segs) {
        kw::launch(g, b, 0, [&] { kb_seg_sum(c, rp, segs); });
        const int64_t len = plan_longest_stream(c, rp.height);
        g_plan_shapes[3] = std::max(g_plan_shapes[3], len); g_plan_shapes[4] = std::max<int64_t>(g_plan_shapes[4], (len + 1 + KPS_SEG - 1) / KPS_SEG); g_plan_shapes[5] = std::max<int64_t>(g_plan_shapes[5], b);
    }
    void seg_gate(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { kw::launch(g, b, 0, [&] { kb_seg_gate(c, rp, segs); }); }
    void seg_keys(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { kw::launch(g, b, 0, [&] { kb_seg_keys(c, rp, segs); }); }
    void seg_max(int g, int b, const KaiCtx& c, RoundParams rp, int segs) { kw::launch(g, b, 0, [&] { kb_seg_max(c, rp, segs); }); }
    void plan_emit(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_plan_emit(c); }); }
    void class_capacity(int g, int b, const KaiCtx& c, int buckets, int levels) { kw::launch(g, b, 0, [&] { kb_class_capacity(c, buckets, levels); }); }
    void fill(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, int l1) { kw::launch(g, b, dyn, [&] { kb_fill(c, rp, l1); }); }
    void bucket_build(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_bucket_build(c); }); }
    // KAI_HOSTSIM_NATIVE_FILL=1: the same algorithm as plain scalar C++ (native_bucket_fill.hpp) on a copy of the sets first — timed, and every output checked against the emulated kernel's
    template <class F> void with_native_shadow(const KaiCtx& c, RoundParams rp, BucketParams bp, F&& run) {
        const bool shadow = std::getenv("KAI_HOSTSIM_NATIVE_FILL") != nullptr;  // (read per launch: a test process sets it for single tests)
        kai_native::NativeFillOut nat;
        if (shadow) kai_native::native_fill_buckets(c, rp, bp, nat);
        run();
        if (!shadow) return;
        const BatchCtx& bt = c.bt; const FillStatus& f = bt.fs[0]; bool same = true;
        same = same && f.n_done == nat.fs.n_done && f.mismatch == nat.fs.mismatch && f.all_dead == nat.fs.all_dead && f.planned == nat.fs.planned && f.decisions == nat.fs.decisions && f.attempted == nat.fs.attempted &&
               f.committed == nat.fs.committed && f.rollbacks == nat.fs.rollbacks && f.ops == nat.fs.ops && f.dead_mask == nat.fs.dead_mask;
        for (size_t i = 0; i < nat.words.size() && same; i++) same = bt.bk_words[i] == nat.words[i];
        if (!same && std::getenv("KAI_HOSTSIM_DEBUG")) std::fprintf(stderr, "native shadow: counters or sets differ\n");
        for (int gi = rp.start; gi < f.n_done && same; gi++) {
            const int x = gi - rp.start;
            same = bt.g_out[gi] == nat.g_out[x] && (nat.g_out[x] != BF_OK || (bt.g_opoff[gi] == nat.g_opoff[x] && bt.g_stmt[gi] == nat.g_stmt[x]));  // (offsets: what the apply kernels read, committed jobs only)
            if (!same && std::getenv("KAI_HOSTSIM_DEBUG")) std::fprintf(stderr, "native shadow: job %d (start %d) flag %d out %d/%d opoff %d/%d stmt %d/%d\n", gi, rp.start, (int)bt.g_flag[gi], (int)bt.g_out[gi], (int)nat.g_out[x], bt.g_opoff[gi], nat.g_opoff[x], bt.g_stmt[gi], nat.g_stmt[x]);
            if (same && nat.g_out[x] == BF_OK && bt.g_flag[gi] != BF_GATE) for (int t = 0; t < bt.g_nt[gi] && same; t++) same = bt.t_node[bt.g_first[gi] + t] == nat.t_node[(size_t)bt.g_first[gi] + t];
        }
        if (!same && std::getenv("KAI_HOSTSIM_DEBUG")) std::fprintf(stderr, "native shadow differs: n_done %d/%d mismatch %d/%d all_dead %d/%d planned %d/%d decisions %lld/%lld attempted %lld/%lld committed %lld/%lld rollbacks %lld/%lld ops %lld/%lld dead %llx/%llx\n",
            f.n_done, nat.fs.n_done, f.mismatch, nat.fs.mismatch, f.all_dead, nat.fs.all_dead, f.planned, nat.fs.planned, (long long)f.decisions, (long long)nat.fs.decisions, (long long)f.attempted, (long long)nat.fs.attempted,
            (long long)f.committed, (long long)nat.fs.committed, (long long)f.rollbacks, (long long)nat.fs.rollbacks, (long long)f.ops, (long long)nat.fs.ops, (unsigned long long)f.dead_mask, (unsigned long long)nat.fs.dead_mask);
        g_native_fill_ms += nat.ms; g_native_fill_launches++; g_native_fill_decisions += nat.fs.decisions; if (!same) g_native_fill_diffs++;
    }
    static bool round_off(const KaiCtx& c) { return c.bt.dev_loop && c.bt.ctl->done; }  // a round enqueued ahead of the loop's end: its kernels leave at once (no shadow, no dump)
    void fill_buckets(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) { if (round_off(c)) return; with_native_shadow(c, rp, bp, [&] { kw::launch(g, b, dyn, [&] { kb_fill_buckets(c, rp, bp); }); }); }
    // KAI_HOSTSIM_FILL_DUMP=<prefix>: inputs and outputs of every fill launch over >= 1 000 planned jobs as <prefix>_<n>.bin (what tools/micro/fill_bench.hip replays on the MI355X)
    static void fill_dump(const KaiCtx& c, RoundParams rp, BucketParams bp, bool outputs) {
        const char* pre = std::getenv("KAI_HOSTSIM_FILL_DUMP"); if (!pre || rp.mode == 1) return;
        const BatchCtx& bt = c.bt; const int V = bt.q_valid[c.Q]; if (V - rp.start < 1000) return;
        static int seq = 0; if (!outputs) seq++;
        char path[512]; std::snprintf(path, sizeof path, "%s_%d.%s", pre, seq, outputs ? "out" : "in");
        FILE* f = std::fopen(path, "wb"); if (!f) return;
        auto w = [&](const void* p, size_t n) { std::fwrite(p, 1, n, f); };
        if (!outputs) {
            int32_t hdr[16] = {0x4b464c31, c.C, c.Q, c.P, V, bp.levels, bp.nw, bp.nw1, bp.n_ok, c.NB, 0, 0, 0, 0, 0, 0}; w(hdr, sizeof hdr); w(&rp, sizeof rp); w(&bp, sizeof bp);
            for (int k = 0; k < 64; k++) { const double q = k < c.C ? c.cls[k].req[KAI_RES_GPU] : 0.0; w(&q, 8); }
            w((const void*)bt.g_flag, (size_t)V); w((const void*)bt.g_first, (size_t)V * 4); w((const void*)bt.g_nt, (size_t)V * 4); w((const void*)bt.g_ucls, (size_t)V * 4);
            w((const void*)bt.t_cls, (size_t)c.P * 4); w((const void*)bt.bk_words, (size_t)bp.levels * bp.nw * 8);
        } else {
            w((const void*)bt.fs, sizeof(FillStatus)); w((const void*)bt.g_out, (size_t)V); w((const void*)bt.g_opoff, (size_t)V * 4); w((const void*)bt.g_stmt, (size_t)V * 4);
            w((const void*)bt.t_node, (size_t)c.P * 4); w((const void*)bt.bk_words, (size_t)bp.levels * bp.nw * 8);
        }
        std::fclose(f);
    }
    void fill_levels(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) { if (round_off(c)) return; fill_dump(c, rp, bp, false); with_native_shadow(c, rp, bp, [&] { kw::launch(g, b, dyn, [&] { kb_fill_levels(c, rp, bp); }); }); fill_dump(c, rp, bp, true); }
    void fill_counts(int g, int b, size_t dyn, const KaiCtx& c, RoundParams rp, BucketParams bp) { if (round_off(c)) return; with_native_shadow(c, rp, bp, [&] { kw::launch(g, b, dyn, [&] { kb_fill_counts(c, rp, bp); }); }); }
    void apply_jobs(int g, int b, const KaiCtx& c, int64_t ops_base, int64_t stmt_base) { kw::launch(g, b, 0, [&] { kb_apply_jobs(c, ops_base, stmt_base); }); }
    void apply_nodes(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_apply_nodes(c); }); }
    void index_from_recs(int g, int b, const KaiCtx& c, const NodeRec* recs, int n_recs, uint64_t* l1k, int32_t* l1n, int nb, int blk0, int blk1) { kw::launch(g, b, 0, [&] { kb_index_from_recs(c, recs, n_recs, l1k, l1n, nb, blk0, blk1); }); }
    void shard_mask_nrec(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_shard_mask_nrec(c); }); }
    void shard_keys(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_shard_keys(c); }); }
    void shard_select(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_shard_select(c); }); }
    void shard_compact(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_shard_compact(c); }); }
    void shard_vbuild(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { kb_shard_vbuild(c); }); }
    void shard_scatter(int g, int b, const KaiCtx& c, int total) { kw::launch(g, b, 0, [&] { kb_shard_scatter(c, total); }); }
    int (*ag_fn)(void*, const void*, void*, int64_t) = nullptr; void* ag_user = nullptr;
    int allgather(const void* send, void* recv, int64_t bytes) { return ag_fn ? ag_fn(ag_user, send, recv, bytes) : (int)KAI_ERR_COMM; }  // the test's gloo all-gather
    // rounds without the host: launches complete where they are made, so the "pinned copies" are plain copies
    RoundCtl rslot[KB_ROUND_SLOTS];
    void round_init(const KaiCtx& c, int remaining, int H0, int policy, int64_t ops_base, int64_t stmt_base) { kw::launch(1, 64, 0, [&] { kb_round_init(c, remaining, H0, policy, ops_base, stmt_base); }); }
    void round_next(const KaiCtx& c) { kw::launch(1, 64, 0, [&] { kb_round_next(c); }); }
    void round_finish(const KaiCtx& c) { kw::launch(1, 64, 0, [&] { kb_round_finish(c); }); }
    void round_begin(int) {}
    int round_post(int slot, const void* src, size_t n) { std::memcpy(&rslot[slot], src, n); return 0; }
    int round_wait(int slot, void* dst, size_t n) { std::memcpy(dst, &rslot[slot], n); return 0; }
    int read(void* dst, const void* src, size_t n) { if (n) std::memcpy(dst, src, n); return 0; }
    int write(void* dst, const void* src, size_t n) { std::memcpy(dst, src, n); return 0; }
    int zero(void* dst, size_t n) { std::memset(dst, 0, n); return 0; }
};

// the session-open, action-init and drain kernels on the emulator (the Launcher of kai_open_kernels.hpp's sequences).  The emulator is one object: calling thread only.
struct SimOpenLauncher {
    template <class P> void fill32(P p, int byte, size_t n) { std::memset((void*)p, byte, n * 4); }
    void node_accounting(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { node_accounting_body(c); }); }
    void pod_accounting_reset(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { pod_accounting_reset_body(c); }); }
    void node_accounting_shared(int g, int b, const KaiCtx& c, const int32_t* np_off, const int32_t* np_pods) { kw::launch(g, b, 0, [&] { node_accounting_shared_body(c, np_off, np_pods); }); }
    void total_nodes(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { total_nodes_body(c); }); }
    void total_foreign(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { total_foreign_body(c); }); }
    void job_usage(int g, int b, const KaiCtx& c, double* jsum) { kw::launch(g, b, 0, [&] { job_usage_body(c, jsum); }); }
    void leaf_usage(int g, int b, const KaiCtx& c, const double* jsum) { kw::launch(g, b, 0, [&] { leaf_usage_body(c, jsum); }); }
    void tree_usage(int g, int b, const KaiCtx& c, const int32_t* h_off, const int32_t* h_nodes, int n_h) { kw::launch(g, b, 0, [&] { tree_usage_body(c, h_off, h_nodes, n_h); }); }
    void fair_share_level(int g, int b, const KaiCtx& c, const int32_t* lvl_parents, int first, int count, double* weight, double* rem_amt, uint8_t* rem_has) { kw::launch(g, b, 0, [&] { fair_share_level_body(c, lvl_parents, first, count, weight, rem_amt, rem_has); }); }
    void qnode_static(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { qnode_static_body(c); }); }
    void index_build(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { index_build_body(c); }); }
    void job_init(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { job_init_body(c); }); }
    void leaf_init(int g, int b, const KaiCtx& c) { kw::launch(g, b, 0, [&] { leaf_init_body(c); }); }
    void drain(int g, int b, const KaiCtx& c, const int32_t* slot_queue) { kw::launch(g, b, 0, [&] { drain_body(c, slot_queue); }); }
};

template <class T> T* own(std::vector<std::vector<char>>& pool, size_t n) {
    pool.emplace_back(std::max<size_t>(n, 1) * sizeof(T), 0);
    return reinterpret_cast<T*>(pool.back().data());
}
// kai_ctx_build.hpp's arena on host memory: one vector per array (an overrun stays visible to a sanitizer), every array of the context recorded as kai_core::AllocRec
// records it, and an array that is allocated WITHOUT being written filled with a byte that is neither 0 nor -1 — so that a read of it shows up here, where the
// library's slab holds whatever the last session left
struct SimArena {
    static constexpr int kPoison = 0x5A;  // (an int32 of it is a large positive number: an index or a group id that cannot go unnoticed)
    struct Rec { size_t field_off; char* base; size_t bytes, live; };  // (live: without the one element of an empty array, which nobody reads)
    std::vector<std::vector<char>>& pool; const KaiCtx& c; std::vector<Rec>* recs = nullptr;
    template <class F> char* take(F& field, size_t n, int byte) {
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(*field);
        pool.emplace_back(bytes, (char)byte); char* p = pool.back().data(); field = (F)p;
        const char* fp = reinterpret_cast<const char*>(&field); const char* c0 = reinterpret_cast<const char*>(&c);
        if (recs && fp >= c0 && fp + sizeof(void*) <= c0 + sizeof(KaiCtx)) recs->push_back({(size_t)(fp - c0), p, bytes, n * sizeof(*field)});
        return p;
    }
    template <class F> void alloc(F& field, size_t n) { take(field, n, kPoison); }
    template <class F> void fill(F& field, size_t n, int byte) { take(field, n, byte); } template <class F> void zero(F& field, size_t n) { take(field, n, 0); }
    template <class F, class T> void upload(F& field, const T* host, size_t n) { static_assert(sizeof(*field) == sizeof(T), "element size"); char* p = take(field, n, 0); if (n) std::memcpy(p, host, n * sizeof(T)); }
    template <class F, class T> void stage(F& field, const T* host, size_t n) { upload(field, host, n); } int flush() { return 0; }
    template <class F, class S> void copy_of(F& field, S src, size_t n) { static_assert(sizeof(*field) == sizeof(*src), "element size"); char* p = take(field, n, kPoison); if (n) std::memcpy(p, src, n * sizeof(*field)); }
    int status() const { return 0; }
};

// the switches of the next sessions, written by the kai_hostsim_set_* exports (host_sim.cpp), and what the last run left for kai_hostsim_last_* / kai_hostsim_multi_stats
// node-sharded run (tests/test_dist_gloo.py): rank / world / offers per class and the all-gather of the test's process group
static int g_sh_rank = 0, g_sh_world = 1, g_sh_k = 0; static int (*g_sh_fn)(void*, const void*, void*, int64_t) = nullptr; static void* g_sh_user = nullptr; static int64_t g_sh_exchanges = 0;
static int g_mw_world = 1; static int64_t g_mw_waves = 0, g_mw_sims_run = 0, g_mw_sims_used = 0, g_mw_replays = 0;  // engines of a victim action (kai_hostsim_set_multi) and what they did
static std::vector<int32_t> g_last_groups;  // PodInfo.GPUGroups[0] of the active fraction pods after the last run
static int64_t g_last_victim_stats[3] = {0, 0, 0};  // scenarios, simulations, filtered scenarios of the last run, summed over its actions (the oracle exports the same: kai_oracle_last_victim_stats)

// The state of a session at one moment, as a harness keeps it "right behind the call": what the read-backs show, and `hidden`, what none of them shows, as int32 words
// (per pod: p_on_node, its status, p_accepted, p_virtual; per pod-set: active_alloc, active_used, alive, pipelined; per job: n_pending, j_tta_valid, j_allocated's bits).
struct StateCopy { std::vector<int32_t> p_status, p_node, hidden; std::vector<double> n_idle, n_rel, n_used; std::vector<QShare> shares; };

struct SimSession {
    const kai_config* cfg = nullptr; const kai_snapshot_soa* s = nullptr;
    SharedPods sp;  // shared GPUs in the engine: one GPU memory size for the whole cluster (the queue-capacity step stays node independent)
    HostPrep prep; bool shared = false; int n_actions_total = 1; bool batch_path = true;
    std::vector<std::vector<char>> pool; KaiCtx c{}; OpenAux aux;  // (aux: the open's arrays outside the context — arguments of the open kernels and of the drain)
    std::vector<SimArena::Rec> recs;  // every array of the context, as kai_core::allocs lists them
    std::string* digest_out = nullptr;  // set before open: what the builder put into every array, and what the open's kernels left in them — the two sets of lines kai_session_open prints under KAI_OPEN_DIGEST
    HostBackend be; std::optional<Engine<HostBackend>> eng;  // the one engine that lives across the session's actions
    struct Rep { std::vector<std::vector<char>> pool; KaiCtx c{}; OpenAux aux; };
    std::vector<Rep> reps;  // further engines of a victim action: replicas of the context, of identical layout
    bool index_stale = false; int64_t batch_rounds = 0, batch_actions = 0, bucket_actions = 0, counts_actions = 0, levels_actions = 0;
    std::chrono::steady_clock::time_point t0;  // (elapsed_ms: from the open's math on)
    KaiCtx& ctx() { return c; }

    // everything up to the first action, as kai_session_open; n_actions: this harness keeps ONE out_ops list for the whole cycle; batch_path false: allocate actions on the
    // sequential engine, as under KAI_HOSTSIM_NO_BATCH
    int open(const kai_config* cfg_, const kai_snapshot_soa* s_, int n_actions, bool batch_path_ = true) {
        if (!cfg_ || !s_ || s_->abi_version != KAI_ABI_VERSION) return KAI_ERR_INVALID_ARG;
        cfg = cfg_; s = s_; n_actions_total = n_actions > 0 ? n_actions : 1; batch_path = batch_path_;
        if (const char* e = std::getenv("KAI_HOSTSIM_MW")) { const int v = std::atoi(e); if (v > 0) g_mw_world = v > KAI_MW_MAX ? KAI_MW_MAX : v; }
        if (!sp.build(*cfg, s)) return KAI_ERR_UNSUPPORTED;
        shared = sp.any;
        std::string err; prep.shared_pods = sp.any ? &sp : nullptr;
        if (prep.build(*cfg, s, err)) return KAI_ERR_INVALID_ARG;
        if (s->pod_flags) { std::vector<int32_t> cnt; flag_legacy_mig_nodes(s, prep, cnt); }
        if (int rc = build_ctx(pool, c, aux, &recs)) return rc;
        if (!lean_equals_full()) return KAI_ERR_STATE;
        digest("kai open digest");
        t0 = std::chrono::steady_clock::now();
        if (int rc = open_kernels()) return rc;
        digest("kai open digest behind the kernels");
        eng.emplace(c, be);
        return KAI_OK;
    }
    void digest(const char* prefix) const {
        if (digest_out) for (const SimArena::Rec& a : recs) {
            uint64_t f = 1469598103934665603ull; for (size_t i = 0; i < a.bytes; i++) { f ^= (unsigned char)a.base[i]; f *= 1099511628211ull; }
            char ln[128]; std::snprintf(ln, sizeof ln, "%s: field %zu bytes %zu fnv %016llx\n", prefix, a.field_off, a.bytes, (unsigned long long)f); *digest_out += ln;
        }
    }
    // kai_session_open does not SEND what a snapshot holds as constants (kai_ctx_build.hpp: the shared-GPU model's per-pod arrays without shared-GPU requests and MIG rows, the
    // identity tables of a snapshot without sub-group trees, "no nominated node") — it writes them where they are read.  That they are what would have been sent is checked here on
    // every snapshot the CPU suite runs: the context built the other way (with / without KAI_OPEN_FULL_UPLOADS) is bytewise equal to this session's
    bool lean_equals_full() const {
        std::vector<std::vector<char>> pool2; KaiCtx c2{}; OpenAux aux2; std::vector<SimArena::Rec> recs2;
        bool ok = build_arrays(pool2, c2, aux2, &recs2, !full_uploads()) == 0 && recs2.size() == recs.size();
        for (size_t i = 0; i < recs.size() && ok; i++) ok = recs2[i].field_off == recs[i].field_off && recs2[i].bytes == recs[i].bytes && std::memcmp(recs2[i].base, recs[i].base, recs[i].live) == 0;
        if (!ok) std::fprintf(stderr, "host_sim: the constants kai_session_open writes on the device differ from what KAI_OPEN_FULL_UPLOADS sends\n");
        return ok;
    }
    static bool full_uploads() { return std::getenv("KAI_OPEN_FULL_UPLOADS") != nullptr; }
    // the context's arrays on `pool` by the library's builder (kai_ctx_build.hpp), ONE out_ops list for the whole cycle (the builder's out_lists)
    int build_arrays(std::vector<std::vector<char>>& pool, KaiCtx& c, OpenAux& aux, std::vector<SimArena::Rec>* recs, bool full) const {
        SimArena arena{pool, c, recs}; CtxBuildOut built;
        ctx_scalars(c, *cfg, s);
        if (int rc = ctx_stage_snapshot(arena, c, s)) return rc;
        return ctx_build(arena, c, aux, CtxBuildIn{*cfg, s, prep, sp, full, n_actions_total}, built);
    }
    // ... then what only this harness does — the solver scratch bound at once, the batch path's pools; a member so that further engines of a victim action get replicas of identical layout
    int build_ctx(std::vector<std::vector<char>>& pool, KaiCtx& c, OpenAux& aux, std::vector<SimArena::Rec>* recs = nullptr) const {
        if (int rc = build_arrays(pool, c, aux, recs, full_uploads())) return rc;
        const int N = c.N, P = c.P, S = c.S, J = c.J, Q = c.Q;
        { size_t bytes = solver_scratch_bytes(N, P, S, J, Q, c.W, c.D + c.T, c.TL, c.G); char* base = own<char>(pool, bytes); solver_scratch_bind(c.sv, base, N, P, S, J, Q, c.W, c.D + c.T, c.TL, c.G); for (int i = 0; i <= c.sv.xr_mask; i++) c.sv.xr_key[i] = -1; c.sv.xr_group = own<int32_t>(pool, (size_t)c.sv.xr_mask + 1); }
        if (int rc = batch_bind(c, prep, [&](size_t bytes) { return (void*)own<char>(pool, bytes); }, [&](void* d, const void* h, size_t n) { std::memcpy(d, h, n); return 0; }, g_sh_world, g_sh_rank, g_sh_k)) return rc;
        if (shared || !batch_path || std::getenv("KAI_HOSTSIM_NO_BATCH")) c.bt.enabled = 0;
        return 0;
    }

    // the session-open kernels in kai_session_open's sequence (kai_open_kernels.hpp open_drive), on the calling thread; in two halves only for the harness-only step between them
    int open_kernels() {
        const int P = c.P, J = c.J, Q = c.Q;
        SimOpenLauncher l; const OpenShape shape{prep.n_levels, prep.lvl_off.data(), prep.n_heights, (uint32_t)c.plugins, shared};
        open_usage_drive(l, c, aux, shape);
        // With fraction pods the queue sums are sums of non-integers and their last bit depends on the order of addition.  The device kernels roll pods
        // up job by job and queue by queue; the reference walks pod by pod up the ancestry in Go-map order (proportion.go:347-401), the oracle in (job,
        // status, pod) order.  KAI_HOSTSIM_POD_ORDER_SUMS=1 makes this harness add in the oracle's order, which takes the order of addition out of a
        // comparison with arbitrary portions (0.2, 0.3 ...): what then still differs is control flow.
        const bool pod_order_sums = shared && (c.plugins & KAI_PLUGIN_PROPORTION) && std::getenv("KAI_HOSTSIM_POD_ORDER_SUMS");
        if (pod_order_sums) {
            for (int q = 0; q < Q; q++) for (int k = 0; k < 3; k++) { QShare& x = c.q_share[(size_t)q * 3 + k]; x.allocated = 0; x.allocated_np = 0; x.request = 0; }
            std::vector<int> ord;
            for (int j = 0; j < J; j++) {
                if (c.j_queue[j] < 0) continue;
                ord.clear(); for (int i = 0; i < c.j_n_pods[j]; i++) ord.push_back(c.j_first_pod[j] + i);
                std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return c.p_status[a] < c.p_status[b]; });
                for (int p : ord) {
                    const int st = c.p_status[p]; const bool al = st_allocated(st) && c.p_accepted[p], pe = st == KAI_POD_PENDING;
                    if (!al && !pe) continue;
                    for (int q = c.j_queue[j]; q >= 0; q = c.q_parent[q]) for (int k = 0; k < 3; k++) {
                        QShare& x = c.q_share[(size_t)q * 3 + k]; const double v = k == 2 ? (al ? c.p_acc_gpu[p] : c.p_pend_gpu[p]) : c.p_req[(size_t)(k == 0 ? KAI_RES_CPU : KAI_RES_MEM) * P + p];
                        x.request += v; if (al) { x.allocated += v; if (!c.j_preempt[j]) x.allocated_np += v; }
                    }
                }
            }
        }
        open_shares_drive(l, c, aux, shape);
        return c.st->fault ? KAI_ERR_UNSUPPORTED : KAI_OK;  // (a node's shared-GPU groups did not take its pods: node_accounting_shared_body)
    }
    void rebuild_index() { SimOpenLauncher l; index_drive(l, c); }
    // A call from outside the actions wrote pods into the session (kai_ops_apply, kai_stale_gang_eviction): what kai_core.hip does on the host behind their kernels
    void state_written(bool non_allocate) { index_stale = true; if (non_allocate) c.fast_ok = 0; }

    // one action of the cycle, as kai_action_execute
    int action(int a) {
        if (a < KAI_ACTION_ALLOCATE || a > KAI_ACTION_PREEMPT) return KAI_ERR_UNSUPPORTED;
        if (a != KAI_ACTION_ALLOCATE && cfg->use_scheduling_signatures && !s->job_signature && c.J > 0) return KAI_ERR_UNSUPPORTED;
        c.action = a; { int d = cfg->queue_depth[a]; c.queue_depth = d > 0 ? d : 0; }
        action_init();
        if (a != KAI_ACTION_ALLOCATE) return victim_action();
        if (int rc = allocate_action()) return rc;
        drain();
        return KAI_OK;
    }
    void action_init() {
        SimOpenLauncher l; action_init_drive(l, c, index_stale);  // as kai_action_execute: the bucket fill keeps the sets current, not the class index
        if (std::getenv("KAI_HOSTSIM_PS")) { int ps = std::atoi(std::getenv("KAI_HOSTSIM_PS")); std::fprintf(stderr, "host_sim: before action %d podset %d active_alloc %d used %d alive %d pipelined %d\n", c.action, ps, c.s_active_alloc[ps], c.s_active_used[ps], c.s_alive[ps], c.s_pipelined[ps]); }
        if (c.st->non_allocate_commits) c.fast_ok = 0;  // as kai_action_execute does after every action
    }
    int victim_action() {
        if (g_sh_world > 1) rebuild_index();  // node-sharded group: replicated action on the whole index
        // victim actions on several engines (kai_engine_solver.inc solve_partial_multi): every engine a thread on its own replica of the context; what must
        // hold afterwards — every replica committed the same operations and ended in the same state — is checked here on every run
        const int G = shared ? 1 : g_mw_world;
        const bool xsh = !shared && g_sh_world > 1 && g_x_on && g_x_fn;  // the waves of this action over the ranks of the group
        const int xcap = xsh ? (g_x_cap > 0 ? g_x_cap : xw_default_cap(g_sh_world, G)) : 0;
        c.mw_xworld = xsh ? g_sh_world : 0; c.mw_xrank = xsh ? g_sh_rank : 0; c.mw_xcap = xcap; c.mw_mail = nullptr;
        if (xsh) g_xs.begin(g_sh_world, g_sh_rank, xcap);
        if (G <= 1 && !xsh) { c.mw = nullptr; c.mw_rank = 0; c.mw_world = 1; if (std::getenv("KAI_HOSTSIM_FRESH")) { HostBackend bf; Engine<HostBackend> ef(c, bf); ef.execute_victim_action(); ef.flush_index(); } else eng->execute_victim_action(); return KAI_OK; }
        if (reps.empty() && G > 1) { reps.resize(G - 1); for (auto& r : reps) { if (int rc = build_ctx(r.pool, r.c, r.aux)) return rc; if (r.pool.size() != pool.size()) return KAI_ERR_DEVICE_FAULT; } }
        static MultiCtx M; std::memset(&M, 0, sizeof M); M.world = G; M.hit[0] = M.hit[1] = 0x7fffffff;
        c.mw = &M; c.mw_rank = 0; c.mw_world = G;
        for (int w = 1; w < G; w++) {
            Rep& r = reps[w - 1];
            for (size_t k = 0; k < pool.size(); k++) { if (r.pool[k].size() != pool[k].size()) return KAI_ERR_DEVICE_FAULT; std::memcpy(r.pool[k].data(), pool[k].data(), pool[k].size()); }
            r.c.action = c.action; r.c.queue_depth = c.queue_depth; r.c.fast_ok = c.fast_ok; r.c.use_index = c.use_index; r.c.all_tracked = c.all_tracked; r.c.bt.enabled = 0;
            r.c.mw = &M; r.c.mw_rank = w; r.c.mw_world = G;
            r.c.mw_xworld = c.mw_xworld; r.c.mw_xrank = c.mw_xrank; r.c.mw_xcap = c.mw_xcap; r.c.mw_mail = nullptr;
        }
        std::vector<std::thread> th;
        for (int w = 1; w < G; w++) th.emplace_back([&, w] { HostBackend bw; Engine<HostBackend> ew(reps[w - 1].c, bw); ew.execute_victim_action(); ew.flush_index(); });  // (flush_index: what DevBackend::finish does when the kernel ends)
        { HostBackend b0; Engine<HostBackend> e0(c, b0); e0.execute_victim_action(); e0.flush_index(); }
        for (auto& t : th) t.join();
        if (xsh) { HostXIo io{&M}; const int rcx = g_xs.finish(io, (c.st->fault || M.fault) ? 1 : 0); g_x_exchanges += g_xs.exchanges; c.mw_xworld = 0; if (rcx && !c.st->fault) return rcx; }
        g_mw_waves += M.waves; g_mw_sims_run += M.sims_run; g_mw_sims_used += M.sims_used; g_mw_replays += M.replays;
        if (int rc = replicas_agree(G)) return rc;
        c.mw = nullptr; c.mw_world = 1;
        return KAI_OK;
    }
    // what must hold behind a victim action on several engines: every replica committed the same operations and ended in the same state as engine 0, bit for bit
    int replicas_agree(int G) const {
        const int N = c.N, P = c.P, J = c.J, Q = c.Q, R = c.R;
        // (tasks-to-allocate caches: an engine may have filled the cache of a bystander job while another has not — the same content whenever it is computed,
        // job_info.go:253-256 invalidates it with every status change of the job's tasks — so: where both hold one, the same one)
        auto tta_same = [&](const KaiCtx& r) { for (int j = 0; j < J; j++) { if (!r.j_tta_valid[j] || !c.j_tta_valid[j]) continue; if (r.j_tta_n[j] != c.j_tta_n[j] || std::memcmp(r.tta + c.j_first_pod[j], c.tta + c.j_first_pod[j], (size_t)c.j_tta_n[j] * 4) != 0 || std::memcmp(r.j_tta_res + (size_t)j * 4, c.j_tta_res + (size_t)j * 4, 24) != 0) return false; } return true; };
        for (int w = 1; w < G; w++) {  // the engines must agree bit for bit
            const KaiCtx& r = reps[w - 1].c;
            bool same = r.st->out_len == c.st->out_len && r.st->fault == c.st->fault && std::memcmp(r.out_ops, c.out_ops, (size_t)c.st->out_len * sizeof(kai_op)) == 0 && std::memcmp(r.p_status, c.p_status, (size_t)P * 4) == 0 &&
                        std::memcmp(r.p_node, c.p_node, (size_t)P * 4) == 0 && std::memcmp(r.n_idle, c.n_idle, (size_t)R * N * 8) == 0 && std::memcmp(r.n_rel, c.n_rel, (size_t)R * N * 8) == 0 &&
                        std::memcmp(r.q_share, c.q_share, (size_t)Q * 3 * sizeof(QShare)) == 0 && tta_same(r) &&
                        r.st->decisions == c.st->decisions && r.st->simulations == c.st->simulations && r.st->scenarios == c.st->scenarios && r.st->scenarios_filtered == c.st->scenarios_filtered;
            if (!same && std::getenv("KAI_HOSTSIM_DEBUG")) {
                std::fprintf(stderr, "host_sim: differs: ops %d status %d node %d idle %d rel %d shares %d tta_valid %d | decisions %lld/%lld sims %lld/%lld scen %lld/%lld filt %lld/%lld\n", std::memcmp(r.out_ops, c.out_ops, (size_t)c.st->out_len * sizeof(kai_op)) != 0, std::memcmp(r.p_status, c.p_status, (size_t)P * 4) != 0, std::memcmp(r.p_node, c.p_node, (size_t)P * 4) != 0,
                             std::memcmp(r.n_idle, c.n_idle, (size_t)R * N * 8) != 0, std::memcmp(r.n_rel, c.n_rel, (size_t)R * N * 8) != 0, std::memcmp(r.q_share, c.q_share, (size_t)Q * 3 * sizeof(QShare)) != 0, std::memcmp(r.j_tta_valid, c.j_tta_valid, (size_t)J * 4) != 0,
                             (long long)r.st->decisions, (long long)c.st->decisions, (long long)r.st->simulations, (long long)c.st->simulations, (long long)r.st->scenarios, (long long)c.st->scenarios, (long long)r.st->scenarios_filtered, (long long)c.st->scenarios_filtered);
                for (int j = 0; j < J; j++) if (r.j_tta_valid[j] != c.j_tta_valid[j]) std::fprintf(stderr, "   job %d tta_valid %d vs %d (pending %d)\n", j, r.j_tta_valid[j], c.j_tta_valid[j], c.j_n_pending[j]);
            }
            if (!same) { if (std::getenv("KAI_HOSTSIM_DEBUG")) std::fprintf(stderr, "host_sim: engine %d of %d ended in another state than engine 0 (ops %lld vs %lld, fault %d vs %d)\n", w, G, (long long)r.st->out_len, (long long)c.st->out_len, r.st->fault, c.st->fault); return KAI_ERR_DEVICE_FAULT; }
        }
        return KAI_OK;
    }
    // the batch path when the action qualifies (kai_batch.hpp), else the sequential engine — as kai_action_execute does
    int allocate_action() {
        HostLauncher hl; BatchStats bs; hl.ag_fn = g_sh_fn; hl.ag_user = g_sh_user;
        if (int rc = batch_allocate(hl, c, prep.shape, bs, c.st->out_len, c.st->stmts)) return rc;
        if (bs.ran) {
            if (!bs.st_on_device) { c.st->decisions += bs.decisions; c.st->jobs_attempted += bs.attempted; c.st->jobs_committed += bs.committed; c.st->rollbacks += bs.rollbacks; c.st->out_len += bs.ops; c.st->stmts += bs.committed;
                                    c.st->drain_pending = bs.drain; }
            batch_rounds += bs.rounds; batch_actions++; bucket_actions += bs.buckets ? 1 : 0; counts_actions += bs.buckets >= 2 ? 1 : 0; levels_actions += bs.buckets == 3 ? 1 : 0;
            if (bs.buckets) index_stale = true;
            g_sh_exchanges = bs.exchanges;
        } else {
            // a node-sharded group shards the batch path's fill; every other action runs replicated on every rank (kai_action.hpp action_engine)
            if (g_sh_world > 1) rebuild_index();  // the sharded fill left an index of the own slice only
            eng->execute_allocate();
        }
        return KAI_OK;
    }
    void drain() { SimOpenLauncher l; drain_drive(l, c, aux); c.st->drain_pending = 0; }  // (the library's scalars start every action from zero; this harness keeps one EngineState for the cycle)

    // ---- behind the last action: the engine's verdict, then the read-backs (nodes in the caller's indices: prep.perm is engine node -> caller's index, prep.rank_of its inverse)
    int finish() const {
        if (std::getenv("KAI_HOSTSIM_DEBUG")) std::fprintf(stderr, "host_sim: scenarios %lld simulations %lld filtered %lld attempted %lld committed %lld decisions %lld sim-queue pops %lld | N %d C %d NB %d NSB %d R %d plugins 0x%x\n", (long long)c.st->scenarios, (long long)c.st->simulations, (long long)c.st->scenarios_filtered, (long long)c.st->jobs_attempted, (long long)c.st->jobs_committed, (long long)c.st->decisions, (long long)c.st->prof[4], c.N, c.C, c.NB, c.NSB, c.R, (unsigned)c.plugins);
#ifdef KAI_PROF_VICTIM
        if (std::getenv("KAI_HOSTSIM_DEBUG")) { std::fprintf(stderr, "host_sim prof:"); for (int i = 0; i < KAI_NPROF; i++) std::fprintf(stderr, " %lld", (long long)c.st->prof[i]); std::fprintf(stderr, "\n"); }
#endif
        if (c.st->fault) { if (std::getenv("KAI_HOSTSIM_DEBUG")) std::fprintf(stderr, "host_sim: engine fault %d at line %d\n", c.st->fault, c.st->fault_line); return KAI_ERR_DEVICE_FAULT; }
        return KAI_OK;
    }
    double elapsed_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    int engine_node(int caller) const { return (int)prep.rank_of[caller]; }
    int caller_node(int n) const { return n >= 0 ? prep.perm[n] : -1; }
    // the first n_keep committed operations (-1: all of them); *n_ops is set also where out is NULL or too small
    int ops(kai_op* out, int64_t cap, int64_t* n_ops, int64_t n_keep = -1) const {
        const int64_t n = n_keep < 0 ? c.st->out_len : n_keep;
        if (n_ops) *n_ops = n;
        if (!out) return KAI_OK;
        if (n > cap) return KAI_ERR_CAPACITY;
        std::memcpy(out, c.out_ops, (size_t)n * sizeof(kai_op)); for (int64_t i = 0; i < n; i++) if (out[i].node >= 0) out[i].node = prep.perm[out[i].node];
        return KAI_OK;
    }
    void put_pods(const int32_t* st, const int32_t* nd, int32_t* status_out, int32_t* node_out) const {
        if (status_out) std::memcpy(status_out, st, (size_t)c.P * 4);
        if (node_out) for (int p = 0; p < c.P; p++) node_out[p] = caller_node(nd[p]);
    }
    void put_shares(const QShare* sh, kai_queue_share* out) const {
        if (out) for (int q = 0; q < c.Q; q++) for (int k = 0; k < 3; k++) { const QShare& x = sh[(size_t)q * 3 + k];
            out[q].fair_share[k] = x.fair; out[q].allocated[k] = x.allocated; out[q].allocated_non_preemptible[k] = x.allocated_np; out[q].request[k] = x.request; out[q].deserved[k] = x.deserved; out[q].max_allowed[k] = x.max_allowed; }
    }
    void put_nodes(const double* idle, const double* rel, const double* used, kai_node_state* out) const {
        const int N = c.N, R = c.R;
        if (out) for (int n = 0; n < N; n++) { kai_node_state& o = out[prep.perm[n]]; std::memset(&o, 0, sizeof(kai_node_state)); for (int r = 0; r < R; r++) { o.idle[r] = idle[(size_t)r * N + n]; o.releasing[r] = rel[(size_t)r * N + n]; o.used[r] = used[(size_t)r * N + n]; } }
    }
    void pod_state(int32_t* status_out, int32_t* node_out) const { put_pods(c.p_status, c.p_node, status_out, node_out); }
    void shares(kai_queue_share* out) const { put_shares(c.q_share, out); }
    void nodes(kai_node_state* out) const { put_nodes(c.n_idle, c.n_rel, c.n_used, out); }
    void publish_last() const {  // for kai_hostsim_last_victim_stats / kai_hostsim_last_gpu_groups
        g_last_victim_stats[0] = c.st->scenarios; g_last_victim_stats[1] = c.st->simulations; g_last_victim_stats[2] = c.st->scenarios_filtered;
        g_last_groups.assign(c.P, -1);
        for (int p = 0; p < c.P; p++) if (shared && c.p_shared[p] && st_active_used(c.p_status[p])) g_last_groups[p] = c.p_group[p];
    }
    void stats(kai_action_stats* stats) const {
        if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->decisions = c.st->decisions; stats->node_scans = c.st->node_scans; stats->nodes_scanned = c.st->nodes_scanned; stats->jobs_attempted = c.st->jobs_attempted; stats->jobs_committed = c.st->jobs_committed; stats->rollbacks = c.st->rollbacks; stats->reserved[0] = c.st->index_queries; stats->reserved[1] = c.st->index_refreshes; stats->reserved[2] = c.st->drained_jobs; stats->reserved[3] = c.st->drained_decisions; stats->reserved[4] = batch_actions; stats->reserved[5] = batch_rounds; stats->reserved[6] = bucket_actions; stats->reserved[7] = counts_actions | (levels_actions << 32); }
    }
    StateCopy snapshot_state() const {
        StateCopy g;
        g.p_status.assign(c.p_status, c.p_status + c.P); g.p_node.assign(c.p_node, c.p_node + c.P);
        g.n_idle.assign(c.n_idle, c.n_idle + (size_t)c.R * c.N); g.n_rel.assign(c.n_rel, c.n_rel + (size_t)c.R * c.N); g.n_used.assign(c.n_used, c.n_used + (size_t)c.R * c.N);
        g.shares.assign(c.q_share, c.q_share + (size_t)c.Q * 3);
        for (int p = 0; p < c.P; p++) { g.hidden.push_back(c.p_on_node[p]); g.hidden.push_back(c.p_on_node[p] >= 0 ? c.p_on_node_status[p] : 0); g.hidden.push_back(c.p_accepted[p]); g.hidden.push_back(c.p_virtual[p]); }
        for (int s = 0; s < c.S; s++) { g.hidden.push_back(c.s_active_alloc[s]); g.hidden.push_back(c.s_active_used[s]); g.hidden.push_back(c.s_alive[s]); g.hidden.push_back(c.s_pipelined[s]); }
        for (int j = 0; j < c.J; j++) { g.hidden.push_back(c.j_n_pending[j]); g.hidden.push_back(c.j_tta_valid[j]); for (int k = 0; k < 3; k++) { int64_t b; std::memcpy(&b, &c.j_allocated[(size_t)j * 4 + k], 8); g.hidden.push_back((int32_t)b); g.hidden.push_back((int32_t)(b >> 32)); } }
        return g;
    }
    // a copy into the caller's output arrays (each may be NULL)
    int write(const StateCopy& g, int32_t* status_out, int32_t* node_out, kai_queue_share* shares_out, kai_node_state* nodes_out, int32_t* hidden = nullptr, int64_t hidden_cap = 0, int64_t* n_hidden = nullptr) const {
        put_pods(g.p_status.data(), g.p_node.data(), status_out, node_out); put_shares(g.shares.data(), shares_out); put_nodes(g.n_idle.data(), g.n_rel.data(), g.n_used.data(), nodes_out);
        if (n_hidden) *n_hidden = (int64_t)g.hidden.size();
        if (hidden) { if ((int64_t)g.hidden.size() > hidden_cap) return KAI_ERR_CAPACITY; std::memcpy(hidden, g.hidden.data(), g.hidden.size() * 4); }
        return KAI_OK;
    }
};

// ---- kai_ops_apply on a session (kai_ops_apply.hpp oa_drive on the emulated lanes): shared by the harnesses whose entry point applies operations
struct ApplyScratch {  // the handle's scratch: zero between calls
    std::vector<int32_t> stamp, sh_status, sh_node;
    void fit(int P) { if ((int)stamp.size() < P) { stamp.assign((size_t)P, 0); sh_status.assign((size_t)P, 0); sh_node.assign((size_t)P, 0); } }
    bool clean(int P) const { for (int p = 0; p < P; p++) if (stamp[p] || sh_status[p]) return false; return true; }
    void bind(OaArgs& a) { a.stamp = stamp.data(); a.sh_status = sh_status.data(); a.sh_node = sh_node.data(); }
};
struct ApplyLauncher {
    void check(int g, int b, const KaiCtx& c, const OaArgs& a) { kw::launch(g, b, 0, [&] { oa_check_body(c, a); }); }
    void wide(int g, int b, const KaiCtx& c, const OaArgs& a) { kw::launch(g, b, 0, [&] { oa_wide_body(c, a); }); }
    int engine(const KaiCtx& c, const OaArgs& a) { KaiCtx cv = c; cv.use_index = 0; HostBackend be; oa_engine_walk(cv, be, a); return 0; }  // as k_oa_engine: one lane, no class index
    int read_head(OaHead& hv, const OaArgs& a) { hv = *a.head; return 0; }
};
// kai_ops_apply from its first device call on (the refusals in front of it are host code of kai_core.hip, tested under tests/host_sim/fake_hip.cpp): src in the caller's node
// indices; -> what the entry point would return, and its result
inline int sim_ops_apply(SimSession& ss, ApplyScratch& sc, const kai_op* src, int n, uint32_t flags, int lanes, kai_apply_result& res) {
    KaiCtx& c = ss.ctx();
    res.first_bad = -1; res.path = KAI_APPLY_PATH_NONE; res.statements = 0;
    if (!n) return KAI_OK;
    sc.fit(c.P);
    std::vector<kai_op> ops(src, src + n); bool non_alloc = false; int statements = 1;
    for (int i = 0; i < n; i++) { ops[i].node = ss.engine_node(ops[i].node); if (ops[i].kind != KAI_OP_ALLOCATE) non_alloc = true; if (i && ops[i].stmt != ops[i - 1].stmt) statements++; }
    OaHead head{}; head.bad = KAI_OA_NONE;
    OaArgs a{}; a.n = n; a.flags = flags | (oa_wide_session(c) ? 0u : KAI_OA_NOT_WIDE); a.use_islot = oa_use_islot(c);
    a.ops = ops.data(); a.head = &head; sc.bind(a);
    ApplyLauncher l; OaHead hv{}; int path = 0;
    int status = oa_drive(l, c, a, lanes, hv, path);
    if (status == KAI_ERR_STATE) res.first_bad = hv.bad;
    if (status == KAI_OK) { res.path = path; res.statements = statements; }
    if (!sc.clean(c.P)) status = KAI_ERR_DEVICE_FAULT;  // the scratch must be clean again
    if (status == KAI_OK && !(flags & KAI_APPLY_CHECK_ONLY)) ss.state_written(non_alloc);
    return status;
}

}  // namespace
