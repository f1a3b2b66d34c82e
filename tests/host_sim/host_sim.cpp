// host_sim.cpp — TEST INFRASTRUCTURE: compiles the engine's control flow (kai_engine.hpp) for the host.
//
// There is no GPU in the development container, so the device engine's sequential control flow
// (kai::Engine<>, the same header the gfx950 kernel instantiates) is additionally compiled here with
// plain g++ and a serial node scanner, to debug it against the oracle in the `-m "not gpu"` suite.
// This is NOT a CPU fallback: libkai_core never contains it, the package never loads it, and every
// parity claim is made by the `-m gpu` tests through the C ABI on a real MI355X.
//
// The session itself (backend, launcher, open, actions, read-backs) is struct SimSession of sim_session.hpp; this file holds the library's exports: whole cycles
// (kai_hostsim_run), the switches of the next runs, and the self-tests that need no session.
#include "sim_session.hpp"

// exhaustive checks of the small arithmetic helpers of kai_fill_levels.hpp (tests/test_batch_path.py): 0 = all hold, else the first failing case as a << 8 | b
extern "C" int kai_hostsim_fill_levels_selfcheck() {
    for (int b = 1; b <= 8; b++) for (int a = 0; a <= 1024; a++) if (kfl_div(a, b) != a / b) return (a << 8) | b;
    for (int lv = 1; lv <= KFL_LMAX; lv++) for (int lane = 0; lane < 64; lane++) { const uint32_t t = kfl_tab(lane, lv); for (int g = 0; g <= lv; g++) if (kfl_quot(t, g) != g / (lane + 1)) return (g << 8) | (lane + 1) | (1 << 30); }
    for (int g = 2; g <= KFL_LMAX; g++) for (int g2 = 1; g2 < g; g2++) { const int p = kfl_pair(g, g2); if (p < 0 || p >= KFL_PAIRS) return (g << 8) | g2 | (1 << 29); for (int h = 2; h <= KFL_LMAX; h++) for (int h2 = 1; h2 < h; h2++) if ((h != g || h2 != g2) && kfl_pair(h, h2) == p) return (g << 8) | g2 | (1 << 28); }
    for (int g = 0; g <= 8; g++) for (int g2 = 0; g2 <= 8; g2++) for (int per = 0; per <= 8; per++) for (int k : {0, 1, 7, 1024}) { const uint64_t c = kfl_cmd(g, g2, k, per, 0x7ffffff0); const int a = (int)(uint32_t)c;
        if ((a & 15) != g || ((a >> 4) & 15) != g2 || ((a >> 8) & 15) != per || ((a >> 12) & 0x7ff) != k || (int)(uint32_t)(c >> 32) != 0x7ffffff0) return (g << 8) | g2 | (1 << 27); }
    return 0;
}
// node-sharded run (tests/test_dist_gloo.py): rank / world / offers per class and the all-gather of the test's process group, for the next run
extern "C" void kai_hostsim_set_shard(int rank, int world, int k, int (*fn)(void*, const void*, void*, int64_t), void* user) { g_sh_rank = rank; g_sh_world = world; g_sh_k = k; g_sh_fn = fn; g_sh_user = user; }
extern "C" int64_t kai_hostsim_last_exchanges() { return g_sh_exchanges; }
// victim actions of a node-sharded run: on = their simulation waves are dealt out over the ranks (kai_victim_shard.hpp) through fn, an all-gather on host memory;
// cap = simulations per wave (0 = the default: two per engine of the group).  Off = every rank runs the whole action (replicated).
extern "C" void kai_hostsim_set_victim_shard(int on, int cap, int (*fn)(void*, const void*, void*, int64_t), void* user) { g_x_on = on; g_x_cap = cap; g_x_fn = fn; g_x_user = user; g_x_exchanges = 0; }
extern "C" int64_t kai_hostsim_victim_exchanges() { return g_x_exchanges; }
extern "C" void kai_hostsim_set_dom_lanes_min(int n) { g_dom_lanes_min = n < 1 ? 1 : n; }
extern "C" void kai_hostsim_set_multi(int engines) { g_mw_world = engines < 1 ? 1 : engines > KAI_MW_MAX ? KAI_MW_MAX : engines; g_mw_waves = g_mw_sims_run = g_mw_sims_used = g_mw_replays = 0; }  // victim actions of the next runs on that many engines
extern "C" void kai_hostsim_multi_stats(int64_t* out) { out[0] = g_mw_waves; out[1] = g_mw_sims_run; out[2] = g_mw_sims_used; out[3] = g_mw_replays; }
extern "C" int kai_hostsim_last_victim_stats(int64_t* out3) { for (int i = 0; i < 3; i++) out3[i] = g_last_victim_stats[i]; return 0; }
extern "C" int kai_hostsim_last_gpu_groups(int32_t* out, int cap) { int n = (int)g_last_groups.size(); for (int i = 0; i < n && i < cap; i++) out[i] = g_last_groups[i]; return n; }
// host clocks of the per-cycle host preparation (HostPrep + SharedPods: what kai_session_open does before the first upload), phase by phase — timing aid
extern "C" int kai_hostsim_prep_ms(const kai_config* cfg, const kai_snapshot_soa* s, double* out, int cap) {
    auto t0 = std::chrono::steady_clock::now();
    // (kept between calls, as kai_core keeps them between sessions: after the first call the arrays are touched memory)
    static SharedPods sp; if (!sp.build(*cfg, s)) return KAI_ERR_UNSUPPORTED;
    auto t1 = std::chrono::steady_clock::now();
    static HostPrep prep; std::string err;
    if (prep.build(*cfg, s, err)) return KAI_ERR_INVALID_ARG;
    auto t2 = std::chrono::steady_clock::now();
    if (cap > 0) out[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (cap > 1) out[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
    for (int i = 0; i < 8 && i + 2 < cap; i++) out[i + 2] = prep.phase_ms[i];
    return 0;
}
// HostPrep::build's verdict on a snapshot: its return code and, for a refused one, the message (what kai_session_open hands to kai_last_error)
extern "C" int kai_hostsim_prep_error(const kai_config* cfg, const kai_snapshot_soa* s, char* msg, int cap) {
    HostPrep prep; std::string err;
    const int rc = prep.build(*cfg, s, err);
    if (msg && cap > 0) { std::snprintf(msg, (size_t)cap, "%s", err.c_str()); }
    return rc;
}
// one cycle: open, the actions, every read-back
extern "C" int kai_hostsim_run(const kai_config* cfg, const kai_snapshot_soa* s, const int* actions, int n_actions,
                               kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, int32_t* pod_status_out, int32_t* pod_node_out,
                               kai_queue_share* shares_open, kai_queue_share* shares_final, kai_node_state* nodes_out,
                               kai_action_stats* stats, double* elapsed_ms_out) {
    SimSession ss;
    if (int rc = ss.open(cfg, s, n_actions)) return rc;
    ss.shares(shares_open);
    for (int i = 0; i < n_actions; i++) if (int rc = ss.action(actions[i])) return rc;
    if (elapsed_ms_out) *elapsed_ms_out = ss.elapsed_ms();
    if (int rc = ss.finish()) return rc;
    if (int rc = ss.ops(ops_out, ops_cap, n_ops)) return rc;
    ss.publish_last();
    ss.pod_state(pod_status_out, pod_node_out); ss.shares(shares_final); ss.nodes(nodes_out); ss.stats(stats);
    return KAI_OK;
}

// what the open's builder (kai_ctx_build.hpp) put into every array of a session's context, as the lines kai_session_open prints under KAI_OPEN_DIGEST (tests/test_open_uploads.py
// holds them against the library's): the text into out, its length into *n also where out is NULL or too small
extern "C" int kai_hostsim_open_digest(const kai_config* cfg, const kai_snapshot_soa* s, char* out, int64_t cap, int64_t* n) {
    SimSession ss; std::string text; ss.digest_out = &text;
    if (int rc = ss.open(cfg, s, 1)) return rc;
    if (n) *n = (int64_t)text.size();
    if (!out) return KAI_OK;
    if ((int64_t)text.size() > cap) return KAI_ERR_CAPACITY;
    std::memcpy(out, text.data(), text.size());
    return KAI_OK;
}

// ---- kai_victim_shard.hpp on its own (tests/test_dist_gloo.py::test_wave_exchange_protocol): R ranks in one process, the "all-gather" a memcpy between their send buffers.
// mode 0: random waves — every rank must end with the identical merged wave, equal to what one rank running every simulation would hold (returns 0, or the failing check).
// mode 1: rank `arg` leaves the protocol (its closing message with the fault flag) while the others are in a wave — they must see the fault, skip their own closing
//         message, and every rank must have issued the same number of collectives.
extern "C" int kai_hostsim_xw_selftest(int R, int cap_in, int mode, int arg, uint64_t seed) {
    using namespace kai;
    if (R < 1 || R > 16) return -1;
    const int cap = xw_cap(cap_in);
    auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(seed >> 33); };
    struct Rank { XShardHost xs; std::vector<int32_t> res; std::vector<int64_t> cnt; int32_t hdr[8]; int hit = 0, xrun = 0, fault = 0, rc = 0; const unsigned char* gathered = nullptr; };
    std::vector<Rank> rk((size_t)R);
    for (int r = 0; r < R; r++) { rk[r].xs.begin(R, r, cap_in); rk[r].res.assign(KAI_MW_WAVE, 0); rk[r].cnt.assign((size_t)KAI_MW_WAVE * KAI_MW_CNT, 0); }
    // the exchange step for all ranks at once: phase 1 every rank packs (wave or closing message), phase 2 every rank merges the same R messages
    std::vector<unsigned char> all(xw_msg_bytes(cap, R) * (size_t)R);
    struct Io { Rank* me; std::vector<unsigned char>* all; int R; int phase;  // phase 0: publish the send buffer, report "not yet"; the driver below re-runs with phase 1
        int pull(int32_t* hdr, int32_t* res, int64_t* cnt, int b, int cap) { std::memcpy(hdr, me->hdr, sizeof me->hdr); std::memcpy(res, me->res.data(), 4 * (size_t)cap); std::memcpy(cnt, me->cnt.data(), 8 * KAI_MW_CNT * (size_t)cap); (void)b; return 0; }
        int push(int b, const int32_t* res, const int64_t* cnt, int cap, int hit, int xrun, int fault) { (void)b; std::memcpy(me->res.data(), res, 4 * (size_t)cap); std::memcpy(me->cnt.data(), cnt, 8 * KAI_MW_CNT * (size_t)cap); me->hit = hit; me->xrun = xrun; me->fault = fault; return 0; }
        int allgather(const void* s, void* r, int64_t n) { if (phase == 0) { std::memcpy(all->data() + (size_t)me->xs.r * (size_t)n, s, (size_t)n); return 1; } std::memcpy(r, all->data(), (size_t)n * R); return 0; } };
    auto exchange = [&](int b, const std::vector<int>& closing) {  // closing[r] = -1: rank r is in a wave; else its closing message with that fault flag; -2: takes no part (already gone)
        for (int phase = 0; phase < 2; phase++) for (int r = 0; r < R; r++) {
            if (closing[r] == -2) continue;
            Io io{&rk[r], &all, R, phase};
            XShardHost snap = rk[r].xs;  // phase 0 only publishes: run it on a copy so that the sequence number advances once
            XShardHost& x = phase == 0 ? snap : rk[r].xs;
            rk[r].rc = closing[r] == -1 ? x.wave(io, b) : x.finish(io, closing[r]);
        }
    };
    if (mode == 0) {
        for (int wave = 0; wave < 50; wave++) {
            const int b = wave & 1, n_run = (int)(rnd() % (uint32_t)(cap + 1));  // simulations 0 .. n_run-1 of this wave were run by their owners
            const int hit = (rnd() % 3) ? (int)(rnd() % (uint32_t)(n_run + 1)) : 0x7fffffff; const int true_hit = (hit < n_run) ? hit : 0x7fffffff;
            std::vector<int32_t> ref_res(KAI_MW_WAVE, 0); std::vector<int64_t> ref_cnt((size_t)KAI_MW_WAVE * KAI_MW_CNT, 0);
            for (int i = 0; i < n_run; i++) { ref_res[i] = (int32_t)(rnd() & 0x1ff); for (int k = 0; k < KAI_MW_CNT; k++) ref_cnt[(size_t)i * KAI_MW_CNT + k] = (int64_t)rnd() - 1000; }
            for (int r = 0; r < R; r++) {
                Rank& me = rk[r]; std::fill(me.res.begin(), me.res.end(), -7); std::fill(me.cnt.begin(), me.cnt.end(), -7);
                int next = 0, own_hit = 0x7fffffff;
                for (int i = r; i < n_run; i += R) { me.res[i] = ref_res[i]; for (int k = 0; k < KAI_MW_CNT; k++) me.cnt[(size_t)i * KAI_MW_CNT + k] = ref_cnt[(size_t)i * KAI_MW_CNT + k]; next++; if (i == true_hit) own_hit = i; }
                next += (int)(rnd() % 3);  // engines whose last fetch found nothing to run
                me.hdr[0] = 1; me.hdr[1] = 0; me.hdr[2] = me.hdr[3] = 0; me.hdr[4] = me.hdr[5] = next; me.hdr[6] = me.hdr[7] = own_hit;
            }
            exchange(b, std::vector<int>((size_t)R, -1));
            for (int r = 0; r < R; r++) {
                const Rank& me = rk[r];
                if (me.rc) return 10 + r;
                if (me.hit != true_hit || me.fault) return 100 + r;
                if (true_hit == 0x7fffffff && me.xrun < std::min(n_run, cap)) return 200 + r;  // everything that was run counts when nothing hit
                const int upto = true_hit != 0x7fffffff ? true_hit + 1 : std::min(std::min(me.xrun, n_run), cap);
                for (int i = 0; i < upto; i++) { if (me.res[i] != ref_res[i]) return 300 + r; for (int k = 0; k < KAI_MW_CNT; k++) if (me.cnt[(size_t)i * KAI_MW_CNT + k] != ref_cnt[(size_t)i * KAI_MW_CNT + k]) return 400 + r; }
            }
        }
        exchange(0, std::vector<int>((size_t)R, 0));
        for (int r = 0; r < R; r++) { if (rk[r].rc) return 500 + r; if (rk[r].xs.exchanges != 51) return 600 + r; }
        return 0;
    }
    // mode 1: two good waves, then rank `arg` is gone
    for (int r = 0; r < R; r++) { Rank& me = rk[r]; me.hdr[0] = 1; me.hdr[1] = 0; me.hdr[4] = me.hdr[5] = 1; me.hdr[6] = me.hdr[7] = 0x7fffffff; }
    exchange(0, std::vector<int>((size_t)R, -1)); exchange(1, std::vector<int>((size_t)R, -1));
    std::vector<int> closing((size_t)R, -1); closing[arg % R] = 1;
    exchange(0, closing);
    for (int r = 0; r < R; r++) {
        if (r == arg % R) { if (rk[r].rc != 0 && R > 1) return 700 + r; continue; }   // the rank that left: its closing message went out
        if (rk[r].rc != 0 || !rk[r].fault) return 800 + r;                            // the others: the wave came back with the fault flag (their engines give up)
        Io io{&rk[r], &all, R, 1};
        if (rk[r].xs.finish(io, 1) != 0) return 900 + r;                              // ... and their own closing message is NOT sent any more
    }
    for (int r = 0; r < R; r++) if (rk[r].xs.exchanges != 3) return 1000 + r;          // the same number of collectives everywhere
    return 0;
}
