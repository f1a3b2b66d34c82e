// kai_fill_levels.hpp — the fill of kai_fill_counts.hpp taken apart further: a counting machine that only decides, ONE WAVEFRONT PER LEVEL for the sets, a bookkeeper for the dead gangs.
//
// kai_fill_counts.hpp split the bucket fill into a counting machine (the planned order over cnt[g] = nodes with g free devices) and two set workers that execute its commands on the
// LDS-resident sets.  Measured on BASELINE config 5 (profiles/r05*, r06*): a single wavefront issues an instruction every 8 – 10 cycles whatever it is, the counting machine spent ≈ 135
// of them on every job that reached it — also on the 40 % of them the plan already predicted dead —, and the two workers were busy 65 – 90 % of the time: either chain bounded the
// kernel at about the same length.  This kernel cuts the work of the wavefront every other one waits for to what DECIDING needs, and gives the rest to wavefronts beside it:
//
//   * Wavefront 0, the counting machine.  Lane j of a stretch of 64 jobs holds job j.  A gang of one class that the plan predicted dead and that does not fit the capacities at the
//     stretch's start is dead for good (capacities only shrink during allocate) and takes no part in the walk.  A walked gang is placed OPTIMISTICALLY on the counts — the lowest
//     non-empty level >= q, whole nodes per step — and its commands are published when its last task has found a level; a gang that runs out of levels is rolled back (counts, mask
//     and ring position) having booked the tasks it placed + 1 decisions, exactly what the capacity rule of kai_fill_counts.hpp books.  So this wavefront keeps no
//     capacities at all.  Outcomes, Statement numbers and operation offsets of a stretch come out of one ballot and one prefix sum at its end.  A command is 8 bytes.
//     This wavefront's chain of dependent instructions is the kernel's length, so the walk is written for the instruction stream it compiles to: the usual gang
//     — one class, 1 .. KFL_SHORT tasks — runs through 31 instructions and two branches, everything but the counts in scalar registers, and stores nothing: the commands of a
//     RUN of such gangs are held in lanes and written to the ring by all lanes at once when the run ends.  What a gang's first step is but for the level's population — the
//     level, the target level, the tasks per node, the nodes it wants, whether that is all of it, whether that is what the plan predicted — is a pure function of the job and
//     of the mask of non-empty levels, so all 64 lanes work it out at once for their own jobs, as one word each: the DECISION TABLE.  The gang reads its word (one lane read),
//     takes k = min(kq, nodes of the level), holds the command, writes two counts and two bits of the mask; one test sends it out of line when that was not all of the gang
//     (the general step, unchanged) or when the mask is no longer the one the table was built for — then the table is rebuilt before the next gang reads its word.  No gang is
//     decided before the counts and the mask it sees are final.  The run is cut in front of the first job whose word says "not as predicted", so the loop tests nothing for it.
//   * Wavefronts 1 .. L, the set workers: level g belongs to wavefront g, alone.  Its words, its two summaries and its first node are that wavefront's uniform state (the word that
//     holds the first node is cached in registers: removing the level's first node — what every command does — reads nothing from LDS while that word lasts; the level's first summary lives in the wavefront's lanes, lane j the word of group j, so an emptied word costs one LDS read and an
//     insertion none).  A worker looks at 64
//     commands at a time, one per lane, and walks the ones that name its level: as the SOURCE it removes the level's first k nodes, writes the tasks' nodes and hands (word, mask) to
//     the target level's worker through the ring of that (source, target) pair; as the TARGET it takes the nodes in when it reaches the command.  Every level sees its removals and
//     insertions in command order; nodes only move DOWN the levels, so the wait-for graph has no cycle (a producer waits only for a consumer that is behind it; the worker that is
//     furthest behind waits for nobody).
//   * Wavefront L + 1, the bookkeeper: what a dead gang books is cap + 1 decisions with the capacity cap[q] = Σ_g (g / q)·cnt[g] AT ITS TURN.  The bookkeeper replays the command stream
//     (lane q − 1 keeps cap[q]: two table look-ups and a multiply-add per command), is told a command's job by the command and a stretch's start by its marker, and books the dead gangs between two walked jobs with one
//     population count — off the chain the other wavefronts wait for.
//
// Results are identical to k_fill_counts / k_fill_buckets (and through them to the oracle): tests/test_batch_path.py and tests/test_gpu_parity.py run the fills against each other, the
// emulator runs this kernel's wavefronts as fibers that really interleave (KW_EMU_ORDER), tests/host_sim shadows every launch with the scalar C++ fill.  Clusters with more than
// eight levels (16-device nodes) or with static class bitmaps stay on k_fill_counts / k_fill_buckets.
#pragma once
#include <type_traits>

#include "kai_fill_counts.hpp"

namespace kai {

constexpr int KFL_LMAX = 8;                                // levels = worker wavefronts
constexpr int KFL_RING = 4096;                             // commands the ring holds (a gang, <= KB_PLACED_MAX commands, is written in full before it is published)
constexpr int KFL_XR = 32;                                 // entries of a hand-over ring
constexpr int KFL_SHORT = 16;                              // a gang of one class with at most this many tasks is "short": it is walked in a run (up to KFL_HELD commands of it held in lanes; one step more sends it the long way)
constexpr int KFL_HELD = 3;                                // commands of a short gang a run holds in lanes under bin-pack (c0 .. c2).  Config 5 at full size, the big round: of 42 742 walked gangs 1 944 take three steps, 38 four, none five (DESIGN.md 5.2d "Steps in lanes"); under spread a third step does not occur there and the run holds two
constexpr int KFL_JOB_SHIFT = 23;                          // a command's bits 23-28: its job's index within the stretch (or-ed in by the counting machine: kfl_cmd knows nothing of it)
constexpr int KFL_PAIRS = KFL_LMAX * (KFL_LMAX - 1) / 2;   // (source level g, target level g2 < g)
// -DKFL_PROF, a worker's clocks per kind of event: 0 one node leaves, its word stays | 1 one node, the word is emptied | 2 several nodes of one word | 3 several nodes over more than
// one word | 4 nodes arrive in the cached word | 5 in an empty word | 6 in another non-empty word | 7 a RUN of insertions taken in lanes (events: runs) | 8 the entries of those
// runs (events: entries; no cycles of their own) | 9 a run sent the serial way because its source was behind (cycles: the look that found it out)
constexpr int KFL_WKINDS = 10;
#ifndef KFL_RUN_MIN
#define KFL_RUN_MIN 2                                      // insertions in front of the next removal that make a run (DESIGN.md 5.2d "Runs of insertions": the replay has a run of two at less than two single insertions)
#endif
// a command, 8 bytes: bits 0-3 g, 4-7 g2, 8-11 per, 12-22 k | the upper word: tbase — the first k nodes of level g take `per` tasks each and move to level g2 (0: no level); their tasks are t_node[tbase ..)
// A word with g = 0 is no command but a stretch's MARKER: the counting machine writes one in front of every stretch's commands.
KW_BODY uint64_t kfl_cmd(int g, int g2, int k, int per, int tbase) { return (uint64_t)((uint32_t)g | ((uint32_t)g2 << 4) | ((uint32_t)per << 8) | ((uint32_t)k << 12)) | ((uint64_t)(uint32_t)tbase << 32); }
struct FlMove { uint64_t mask; int32_t w; int32_t seq; };  // the nodes `mask` of word w (bit 30 of w: the command's last entry); seq = the entry's number in its ring + 1, stored last (release)
struct FlLds {
    uint64_t ring[KFL_RING];
    uint64_t dummy[64];            // where the lanes other than lane 0 put their copy of a command (a store without a branch)
    FlMove x[KFL_PAIRS + 1][KFL_XR];  // (the last one: where a hand-over to no level goes — a store without a branch, nobody reads it)
    FlMove xdummy[64];             // ... and where the lanes other than lane 0 put their copy of a hand-over entry
    int32_t xtail[KFL_PAIRS];      // entries the pair's consumer has taken
    int32_t cnt0[KBK_GMAX];
    int32_t tail[KFL_LMAX + 1];    // commands worker g (index g − 1) / the bookkeeper (index KFL_LMAX) has passed
    int32_t head, done, fin, b_dec;  // fin: jobs of the planned order the counting machine executed (for the bookkeeper's last stretch); b_dec: the bookkeeper's decisions
    int64_t w_idle[KFL_LMAX + 1], w_total[KFL_LMAX + 1];  // (the clocks: profiling)
#ifdef KFL_PROF
    int64_t wk_cyc[KFL_LMAX][KFL_WKINDS], wk_cnt[KFL_LMAX][KFL_WKINDS];  // a worker's cycles and events per kind of event
#endif
};
#if defined(KFL_PROF) && defined(__HIPCC__)
__device__ int64_t kfl_prof_workers[KFL_LMAX][KFL_WKINDS + 1][2];  // [level − 1][kind] = cycles, events; [level − 1][KFL_WKINDS] = idle, total (read by tools/micro/fill_bench.hip)
#endif
KW_BODY int kfl_pair(int g, int g2) { return (g - 1) * (g - 2) / 2 + (g2 - 1); }
// a / b for 0 <= a <= 1024, 1 <= b <= 8 on the scalar unit: a·ceil(2^15 / b) >> 15 (the error a·(ceil − exact) / 2^15 stays below 1/32, the fraction of a / b below 7/8)
KW_BODY int kfl_div(int a, int b) {
    const uint64_t inv = b <= 4 ? 0x2000'2AAB'4000'8000ull : 0x1000'124A'1556'199Aull;  // ceil(32768 / b), 16 bits each: b = 1..4 / 5..8
    return (int)(((uint32_t)a * (uint32_t)((inv >> (16 * ((b - 1) & 3))) & 0xffff)) >> 15);
}
// uniform accesses of a worker to its own level's LDS words: every lane reads the same address and takes lane 0's value (a scalar from then on); lane 0 writes
KW_BODY uint64_t kfl_read(KW_LDS_PTR(uint64_t) p) { return kw::bcast(*p, 0); }
KW_BODY void kfl_write(KW_LDS_PTR(uint64_t) p, uint64_t v, KW_LDS_PTR(uint64_t) dummy) { KW_LDS_PTR(uint64_t) q = kw::lane() == 0 ? p : dummy + kw::lane(); *q = v; }  // (the other lanes into a slot of their own: one store, no branch)
// a counter another wavefront publishes (acquire), as a scalar: every lane reads the same address
KW_BODY int kfl_load(const int32_t* p) { return kw::uni(kw::lds_load_acq(p)); }
// one stretch of 64 planned jobs as the counting machine and the bookkeeper both see it: lane j holds job j
struct FlStretch { int flag, first, nt, q; bool valid, is_def; uint64_t defm, todo; };
// lane q − 1: the quotients g / q for g = 1 .. 8, four bits each (bits 4(g − 1) ..)
KW_BODY uint32_t kfl_tab(int lane, int LV) { uint32_t t = 0; for (int g = 1; g <= LV; g++) t |= (uint32_t)(g / (lane + 1)) << (4 * (g - 1)); return t; }
KW_BODY int kfl_quot(uint32_t tab, int g) { return g >= 1 ? (int)((tab >> (4 * (g - 1))) & 15u) : 0; }
// classifies a stretch from its jobs' parameters and the capacities at its start (lane q − 1: capq).  qk: lane k = devices class k asks for.
KW_BODY void kfl_classify(FlStretch& s, int ucls, int qk, int capq) {
    int q = kw::shfl(qk, ucls >= 0 ? ucls : 0);  // devices the job's one class asks for; 0 = a gang of several classes
    if (ucls < 0 || q > 31) q = ucls < 0 ? 0 : 31;  // (a request beyond every level: no level, no capacity)
    const int cap = kw::shfl(capq, q >= 1 ? q - 1 : 63);  // (lane 63 asks for 64 devices: capacity 0)
    s.q = q;
    // dead for good: a gang of one class the plan predicted dead that the levels cannot hold now (the capacities only shrink).  It books cap + 1 decisions at its turn.
    s.is_def = s.valid && s.flag == BF_DEAD && q >= 1 && cap < s.nt;
    s.defm = kw::ballot(s.is_def);
    s.todo = kw::ballot(s.valid && s.flag != BF_GATE && !s.is_def);
}

// SP: the classes' strategy on the GPU as a compile-time parameter (0 bin-pack, 1 spread).  Under spread every class's best node is the first node of the HIGHEST non-empty
// level g (it fits iff g >= q) and takes ONE task before it moves to g − q: the command "(g, g − q, k = min(rest, nodes of g), per = 1)" — no quotient, no division.  The top
// level strictly falls from step to step, capacities and the bookkeeper's replay are what they are under bin-pack.  Workers, bookkeeper, markers, the
// command's format and the rings do not know the strategy.
template <int SP>
KW_BODY void kb_fill_levels_t(const KaiCtx& c, RoundParams rp, BucketParams bp) {
    if (kb_round_off(c.bt)) return;
    KW_SHARED FlLds L;
    const BatchCtx& b = c.bt;
    const int tid = kw::tid(), T = kw::bdim(), lane = kw::lane(), C = c.C;
    BkView v; v.NW = bp.nw; v.NW1 = bp.nw1; v.LV = bp.levels;
    unsigned char* dyn = kw::dyn_lds();
    v.gw = (KW_LDS_PTR(uint64_t))dyn; v.s1 = v.gw + (size_t)v.LV * v.NW; v.ok = v.s1 + (size_t)v.LV * v.NW1 + KBK_GMAX;
    const int64_t tstart = kw::clock();
    if (tid < KBK_GMAX) L.cnt0[tid] = 0;
    if (tid <= KFL_LMAX) { L.tail[tid] = 0; L.w_idle[tid] = 0; L.w_total[tid] = 0; }
    if (tid < KFL_PAIRS) L.xtail[tid] = 0;
#ifdef KFL_PROF
    if (tid < KFL_LMAX * KFL_WKINDS) { L.wk_cyc[tid / KFL_WKINDS][tid % KFL_WKINDS] = 0; L.wk_cnt[tid / KFL_WKINDS][tid % KFL_WKINDS] = 0; }
#endif
    for (int i = tid; i < (KFL_PAIRS + 1) * KFL_XR; i += T) L.x[i / KFL_XR][i % KFL_XR].seq = 0;
    if (tid == 0) { L.head = 0; L.done = 0; L.fin = 0; L.b_dec = 0; }
    for (int i = tid; i < v.LV * v.NW; i += T) v.gw[i] = b.bk_words[i];
    kw::sync();
    for (int i = tid; i < v.LV * v.NW1; i += T) {  // first summary level, and the levels' populations on the way
        const int l = i / v.NW1, w1 = i % v.NW1; uint64_t m = 0; int pop = 0;
        for (int j = 0; j < 64 && w1 * 64 + j < v.NW; j++) { const uint64_t x = v.gw[l * v.NW + w1 * 64 + j]; if (x) { m |= 1ull << j; pop += __builtin_popcountll(x); } }
        v.s1[i] = m;
        if (pop) kw::atomic_add((int32_t*)&L.cnt0[l], pop);
    }
    kw::sync();
    const int V = rp.mode != 1 ? b.q_valid[c.Q] : 0;  // mode 1: dead classes only (before the first plan)
    int64_t my_runs = 0;  // -DKFL_RUN_STATS (tests/test_fill_levels_insert_runs.py builds the emulated replay with it; the product carries none of it): a worker's runs of insertions, taken in lanes | sent the serial way << 32, summed into FillStatus.rescans3 at the end
    const int wave = kw::uni(tid >> 6);  // (the compiler takes anything computed from the thread's number for different in every lane: told otherwise, a wavefront's role, its level and its tests sit on the scalar unit)
    if (wave == 0) {
        // ------------------------------------------------------------------ wavefront 0: the counting machine.
        // lane g: cnt = nodes of level g (lane 0: nodes that left for no level, see KFL_EVENT — a command's g and g2 are lane numbers as they stand).  lane q − 1: tab = the quotients
        // g / q.  lane k: qk = devices class k asks for.
        // lane b − 1: invq = ceil(2^15 / b), the table of kfl_div (b = 1: a·2^15 >> 15 = a, so the step divides without asking whether it has to).
#ifdef KFL_PRIO
        kw::set_prio<KFL_PRIO>();  // (an experiment on placement, DESIGN.md 5.2d: no gain measured, off in the product)
#endif
        int cnt = lane >= 1 && lane <= v.LV ? L.cnt0[lane - 1] : 0;
        const bool act = lane < C;
        const int qk = act ? (int)c.cls[lane].req[KAI_RES_GPU] : 0x7fffffff;
        const uint32_t tab = kfl_tab(lane, v.LV);
        const int invq = (int)(((lane < 4 ? 0x2000'2AAB'4000'8000ull : 0x1000'124A'1556'199Aull) >> (16 * (lane & 3))) & 0xffff);
        uint32_t nz = (uint32_t)kw::ballot(cnt > 0) | 1u;  // bit g: level g holds a node (bit 0, "no level", is always set: a node that leaves for no level sets it again)
        int decisions = 0, attempted = 0, committed = 0, rollbacks = 0, ops = 0, n_done = rp.start, mismatch = 0;
        int wp = 0, tail_seen = 0, pub = 0, n_mark = 0;  // commands written (the stretches' markers, n_mark, among them) / the slowest reader's progress as last read / commands published (per 64 commands and at the end of a stretch)
        int64_t a_wait = 0;               // cycles this wavefront waited for room in the ring
#ifdef KFL_PROF
        int64_t pc[5] = {0, 0, 0, 0, 0}; int64_t pt = kw::clock();
        #define KFL_T(i) do { const int64_t n_ = kw::clock(); pc[i] += n_ - pt; pt = n_; } while (0)
#else
        #define KFL_T(i) (void)0
#endif
        // the slowest reader's progress: lanes 0 .. LV − 1 the workers', lane LV the bookkeeper's
        auto tails_min = [&]() { int t = lane <= v.LV ? kw::lds_load_acq(&L.tail[lane < v.LV ? lane : KFL_LMAX]) : 0x7fffffff; for (int l = 1; l <= v.LV; l++) { const int o = kw::bcast(t, l); t = o < t ? o : t; } return kw::bcast(t, 0); };
        // the lowest non-empty level >= qc (spread: the highest non-empty level, if it is >= qc), 0 = none
        #define KFL_LEVEL_FOR(qc) (((nz >> 1) >> ((qc) - 1)) ? (SP ? 31 - __builtin_clz(nz) : (qc) + __builtin_ctz((nz >> 1) >> ((qc) - 1))) : 0)
        // room for n more commands in the ring (a gang stays unpublished until its last task has found a level)
        #define KFL_ROOM(n) do { if (wp - tail_seen > KFL_RING - (n)) { kw::lds_store_rel(&L.head, wp); pub = wp; const int64_t w0 = kw::clock(); while (wp - tail_seen > KFL_RING - (n)) { tail_seen = tails_min(); if (wp - tail_seen > KFL_RING - (n)) kw::relax(); } a_wait += kw::clock() - w0; } } while (0)
        // lane 0 writes the command, the other lanes a copy into a slot of their own: one store, no branch.  jbits: the job's index within its stretch at bits 23-28 (for the bookkeeper)
        #define KFL_EMIT(g_, g2_, k_, per_, tb_) do { KW_LDS_PTR(uint64_t) sl_ = lane == 0 ? (KW_LDS_PTR(uint64_t))&L.ring[wp & (KFL_RING - 1)] : (KW_LDS_PTR(uint64_t))&L.dummy[lane]; *sl_ = kfl_cmd(g_, g2_, k_, per_, tb_) | jbits; wp++; } while (0)
        // k nodes leave level g, which holds cg >= k, for level g2 (0: none): two lanes of the counts are written, two bits of the non-empty mask change (bit g goes when the level
        // is emptied, bit g2 comes: one scalar instruction each) — all of it on the scalar unit.  Nodes that leave for no level are counted in lane 0, whose bit is always set; a
        // step without a level (g = 0, k = 0, g2 <= 0) adds nothing to any lane, and the gang it belongs to is rolled back.  (Bit 31 of the mask is never set: "clear nothing".)
        #define KFL_EVENT(g_, g2_, k_, cg_) do { const int e_g = (g_), e_g2 = (g2_) > 0 ? (g2_) : 0, e_k = (k_), e_cg = (cg_); \
            const int e_t = kw::bcast(cnt, e_g2 & 63); \
            cnt = kw::writelane(cnt, e_cg - e_k, e_g & 63); \
            cnt = kw::writelane(cnt, e_t + e_k, e_g2 & 63);  /* (read before the source's lane is written: g2 = g only without a level, where k = 0) */ \
            nz = kw::bit_set(kw::bit_clear(nz, e_cg == e_k ? e_g : 31), e_g2); } while (0)
        // one step of a gang of ONE class, whole nodes: the lowest non-empty level g >= q holds r = g / q of its tasks per node; the first k nodes of it take r tasks each and move to
        // level g mod q, a remainder of fewer than r tasks goes to one node, which then stays at level g − rem·q.  No level: the step moves nothing and the gang has failed (it writes
        // a slot that stays unpublished: whatever its fields hold).
        // Spread: g is the highest non-empty level (the highest set bit of nz; `ok` says g >= q), r = 1: the first k = min(rest of the gang, nodes of the level) nodes take one task
        // each and move to g − q — no quotient table, no division.
        #define KFL_STEP(S, EMIT) \
            const uint32_t lv##S = nz >> qc; \
            ok = kw::nonzero01(lv##S);  /* a level >= q holds a node — as a number, not as a comparison (kai_simt.hpp) */ \
            const int g##S = lv##S ? (SP ? 31 - __builtin_clz(nz) : qc + __builtin_ctz(lv##S)) : 0; \
            int r##S = SP ? 1 : (int)((tq >> ((4 * g##S - 4) & 31)) & 15u); r##S = r##S > 1 ? r##S : 1;  /* kfl_quot(tq, g), at least 1 (no level: whatever, nothing moves) */ \
            const int rem##S = nt - placed; \
            const int kq##S = SP ? rem##S : (int)(((uint32_t)rem##S * (uint32_t)kw::bcast(invq, r##S - 1)) >> 15);  /* = kfl_div(rem, r): whole nodes the rest of the gang fills (0: a remainder of fewer than r tasks, on one node) */ \
            const int cg##S = kw::bcast(cnt, g##S & 63); \
            int k##S = kq##S < cg##S ? kq##S : cg##S; k##S = (k##S > 1 ? k##S : 1) * ok;  /* min(kq, nodes of the level), at least the one node; no level: nothing moves */ \
            const int per##S = r##S < rem##S ? r##S : rem##S, g2##S = g##S - per##S * qc; \
            EMIT(g##S, g2##S, k##S, per##S); \
            KFL_EVENT(g##S, g2##S, k##S, cg##S); \
            placed += k##S * per##S
        #define KFL_EMIT_RING(g_, g2_, k_, per_) KFL_EMIT(g_, g2_, k_, per_, first + placed)
        // a command's lower word without its job's index, held in lane jj of a register until the run is flushed (a gang that fails holds whatever: it is never stored)
        #define KFL_LOW(g_, g2_, k_, per_) (int)((uint32_t)(g_) | ((uint32_t)(g2_) << 4) | ((uint32_t)(per_) << 8) | ((uint32_t)(k_) << 12))
        #define KFL_HOLD1(g_, g2_, k_, per_) c1 = kw::writelane(c1, KFL_LOW(g_, g2_, k_, per_), jj)
        #define KFL_HOLD2(g_, g2_, k_, per_) c2 = kw::writelane(c2, KFL_LOW(g_, g2_, k_, per_), jj)
        constexpr int HELD = SP ? 2 : KFL_HELD;  // (statically unrolled below: there is no indexed register access)
        static_assert(KFL_HELD == 3, "c0 .. c2: one more held command is one more register, one more step and one more store below");
        // THE DECISION TABLE: lane j holds the first step of job j under the mask nz_tab, as one word — all that the step is but the level's population: bits 0-11 the command's
        // lower word as it stands (g, g2, per; g = 0: no level >= q holds a node), bits 23-27 kq = the nodes the gang wants of the level (at least 1; the command's k = min(kq,
        // nodes of the level) goes to bits 12-22, which the word leaves empty), bit 28: kq nodes are NOT all of the gang (so bits 23-28 as one number equal k iff one step places
        // it), bit 29: a level was found, bit 30: which is not what the plan predicted.  Built by all lanes at once from the uniform mask and the lane's own job (short gangs
        // only: the other lanes hold whatever), with kfl_div as plain per-lane arithmetic; exact for the mask it was built for, and rebuilt before the next gang reads its word
        // whenever the mask differs (nz_tab == nz is the run's invariant).  mism: the jobs whose word has bit 30 set.
        #define KFL_TABLE() do { \
            const int t_q = s.q >= 1 ? s.q : 1, t_nt = s.nt; \
            const uint32_t t_lv = nz >> t_q; \
            const int t_g = SP ? 31 - __builtin_clz(nz) : t_q + __builtin_ctz(t_lv | 0x80000000u); \
            int t_r = SP ? 1 : (int)((my_tq >> ((4 * t_g - 4) & 31)) & 15u); t_r = t_r > 1 ? t_r : 1; \
            const int t_kq = SP ? t_nt : kfl_div(t_nt, t_r), t_kq1 = t_kq > 1 ? t_kq : 1; \
            const int t_per = t_r < t_nt ? t_r : t_nt, t_g2 = t_g - t_per * t_q; \
            const uint32_t t_p = s.flag == BF_OK ? 1u : 0u; \
            const uint32_t t_w = (uint32_t)t_g | ((uint32_t)t_g2 << 4) | ((uint32_t)t_per << 8) | ((uint32_t)t_kq1 << 23) | (t_kq1 * t_per < t_nt ? 1u << 28 : 0u) | (1u << 29) | ((t_p ^ 1u) << 30); \
            dw = t_lv ? t_w : t_p << 30; nz_tab = nz; mism = kw::ballot(((dw >> 30) & 1u) != 0); } while (0)
        // of the jobs h, the ones up to the first whose word says "ends differently from its prediction" stay in h (that job is the round's last unless a second step or a new
        // table says otherwise), the ones behind it wait in `held`: the loop tests nothing per gang for it
        #define KFL_CUT(h) do { const uint64_t c_m = (h) & mism, c_keep = c_m ? ((c_m & (0 - c_m)) << 1) - 1 : ~0ull; held = (h) & ~c_keep; (h) &= c_keep; } while (0)
        // the end of a gang that went the long way: its outcome bit, what it placed before it failed (a stretch's decisions and rollbacks are summed up at its end: every task of a
        // committed gang is a decision, a gang that found no node for its next task booked the ones it placed and that one), Statement.Rollback (nothing was published: the counts, the
        // mask and the ring position), and whether it ended as predicted
        #define KFL_GANG_END() \
            okm |= (uint64_t)(uint32_t)(1 - fail) << jj; failm |= (uint64_t)(uint32_t)fail << jj; \
            extra += placed & (0 - fail); \
            cnt = fail ? cnt_s : cnt; nz = fail ? nz_s : nz; wp = fail ? wp_s : wp; \
            const int g_mis = (int)((uint32_t)(flag - 1) >> 31) ^ fail ^ 1;  /* (flag == BF_OK) != ok — the job ended differently from its prediction: it is the round's last */ \
            mismatch |= g_mis; last_jj = jj
        // the 64 jobs of a stretch: one per lane; the NEXT stretch's loads are issued before this stretch is walked
        int nx_flag = 0, nx_first = 0, nx_nt = 0, nx_ucls = 0;
        uint32_t dw = 0, nz_tab = ~0u; uint64_t mism = 0;  // the decision table, the mask it was built for (~0: none — a new stretch's jobs) and its mispredicted jobs
        if (V > rp.start) { const int gc = rp.start + lane < V ? rp.start + lane : V - 1; nx_flag = b.g_flag[gc]; nx_first = b.g_first[gc]; nx_nt = b.g_nt[gc]; nx_ucls = b.g_ucls[gc]; }
        for (int base = rp.start; base < V && !mismatch; base += 64) {
            const int gi = base + lane;
            FlStretch s; s.valid = gi < V;
            s.flag = s.valid ? nx_flag : (int)BF_GATE; s.first = s.valid ? nx_first : 0; s.nt = s.valid ? nx_nt : 0;
            const int my_ucls = s.valid ? nx_ucls : 0;
            { const int gc = gi + 64 < V ? gi + 64 : V - 1; nx_flag = b.g_flag[gc]; nx_first = b.g_first[gc]; nx_nt = b.g_nt[gc]; nx_ucls = b.g_ucls[gc]; }
            const int jn = V - base < 64 ? V - base : 64;
            int capq = 0;  // lane q − 1: the tasks that ask for q devices the levels hold at the stretch's start
            for (int g = 1; g <= v.LV; g++) capq += kfl_quot(tab, g) * kw::bcast(cnt, g);
            kfl_classify(s, my_ucls, qk, capq);
            // a job's parameters in one word: flag (2 bits), devices (5 bits), tasks (up to KB_PLACED_MAX: 11 bits), bit 19: predicted to fit, bit 18: the long way (several classes, more tasks than the
            // stretch's reservation in the ring covers, or none at all: the short way takes its first step without asking)
            const int my_pack = s.flag | (s.q << 2) | (s.nt << 7) | ((s.q == 0 || s.nt > KFL_SHORT || s.nt < 1) ? 1 << 18 : 0) | (s.flag == BF_OK ? 1 << 19 : 0);
            const uint32_t my_tq = kw::shfl(tab, s.q >= 1 ? s.q - 1 : 63);  // the quotients g / q of the job's request
            uint64_t longm = kw::ballot(((my_pack >> 18) & 1) != 0);
            nz_tab = ~0u;
            uint64_t todo = s.todo, okm = 0, failm = 0;  // okm / failm: jobs of this stretch that committed / that were walked and found no room
            int n_out = jn, last_jj = 0, extra = 0;  // extra: tasks the failed gangs had placed before they failed
            attempted += jn; n_done = base + jn;
            KFL_ROOM(1);  // room for the stretch's marker (a run asks for the room of its commands when it is flushed, a long gang before it starts: no check per gang)
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("s_waitcnt lgkmcnt(0)" :: "v"(my_tq), "v"(my_pack) : "memory");  // the stretch's shuffles have landed: the walk below never waits on the LDS counter (its own command stores stay in flight)
#endif
            // the stretch's marker, in ring order in front of its commands: the bookkeeper enters the stretch there (no worker looks at it: it names no level)
            { KW_LDS_PTR(uint64_t) sl_ = lane == 0 ? (KW_LDS_PTR(uint64_t))&L.ring[wp & (KFL_RING - 1)] : (KW_LDS_PTR(uint64_t))&L.dummy[lane]; *sl_ = 0; wp++; n_mark++; }
            KFL_T(0);
            // (a conditional branch costs this wavefront 22 - 31 cycles whether it is taken or not, a scalar instruction 5 - 6, a dependent vector instruction 7, a vector compare that
            // feeds the scalar unit 30 — tools/micro/issue_rate.hip.  So the usual gang — one class, 1 .. KFL_SHORT tasks — runs straight through: the short gangs in front of the next
            // long one, a RUN, are walked by a loop that holds nothing else: the first step read from the decision table, ONE rarely taken branch for "a second step or a new table", and
            // the loop's own test (the run is cut in front of the first job the table says is predicted wrong).  Everything but the counts and the table lives in scalar registers.
            // A run stores nothing: the lower word of a gang's command goes into lane jj of c0, that of a second step into c1, and the run is FLUSHED at its end — every lane forms
            // the upper words and the job bits of its own gang's commands, a prefix sum gives it their place in the ring, head is published once.  The ring receives the words in
            // the jobs' order, as if every gang had written its own.  A first step that finds no level moves nothing (k = 0), so only a gang that takes a second step needs the
            // state in front of it: rebuilt there from the first step's values, once, whatever the number of steps behind it.  Under bin-pack a third step goes into c2 the same
            // way (KFL_HELD = 3; lane jj of nx counts the commands beyond the second) and the flush stores a lane's commands one behind the other; a short gang that needs one
            // step more than the lanes hold leaves the run and goes the long way from the start.)
            while (todo) {
                const uint64_t lm = todo & longm;
                const uint64_t below = lm ? (lm & (0 - lm)) - 1 : ~0ull;  // the jobs in front of the next long one
                uint64_t hot = todo & below;
                todo &= ~below;
                if (hot) {
                    const uint64_t run0 = hot; uint64_t twor = 0, rest = 0, fail2 = 0, held;  // the run's jobs / the ones among them that committed with two or more commands / the ones a step beyond the held ones left unwalked / the ones a later step rolled back / the ones behind the first job the table says ends differently from its prediction
                    // (held != 0 only while the last job of `hot` is one the table says is predicted wrong: KFL_CUT is the only place that fills it, and every path that changes the
                    // table, or that job's outcome, either empties it or cuts again.  The jobs of a run are hot | held | the ones walked | rest at any time.)
                    int c0 = 0, c1 = 0, c2 = 0, nx = 0, jj; uint32_t w;  // (nx, lane jj: the commands gang jj holds beyond its second)
                    if (nz != nz_tab) { KFL_TABLE(); }  // (a new stretch, or a long gang changed the mask)
                    KFL_CUT(hot);
                    do {
                        jj = __builtin_ctzll(hot); hot = kw::bit_clear(hot, jj);
                        w = kw::bcast(dw, jj);
                        KFL_T(1);
                        // the gang's first step as the table has it: k = min(kq, nodes of the level) nodes of level g move to g2 (no level: g = g2 = kq = 0, nothing moves)
                        const int g = w & 15, g2 = (w >> 4) & 15;
                        const int cg = kw::bcast(cnt, g), t2 = kw::bcast(cnt, g2);
                        const int kq = (w >> 23) & 31, k = kq < cg ? kq : cg;
                        c0 = kw::writelane(c0, (int)(w | ((uint32_t)k << 12)), jj);
                        cnt = kw::writelane(cnt, cg - k, g);
                        cnt = kw::writelane(cnt, t2 + k, g2);
                        nz = kw::bit_set(kw::bit_clear(nz, cg == k ? g : 31), g2);
                        // out of line, one test for both: the step did not place the whole gang (k is not the kq of a word that says "kq nodes are all of it") | the mask is no longer the table's
                        // (as ONE number the compiler knows nothing about: left to itself it keeps the two comparisons apart, as three lane masks and their conjunction)
                        if (__builtin_expect(kw::opaque((uint32_t)(k ^ (int)((w >> 23) & 63)) | (nz ^ nz_tab)) != 0, 0)) {
                            if (k != (int)((w >> 23) & 63)) {
                                const int pack = kw::bcast(my_pack, jj);
                                const uint32_t tq = kw::bcast(my_tq, jj);
                                const int qc = (pack >> 2) & 31, nt = (pack >> 7) & 0x7ff, pred = (pack >> 19) & 1;
                                const uint32_t nz_s = nz_tab;  // (the mask in front of the gang: the table was built for it)
                                int placed = k * (int)((w >> 8) & 15), ok;
                                // the counts in front of the gang: the first step taken back
                                int cnt_s = kw::writelane(cnt, t2, g2); cnt_s = kw::writelane(cnt_s, cg, g);
                                KFL_STEP(B, KFL_HOLD1);
                                // further steps, in place: each one's lower word into the next held register.  cnt_s / nz_s, kept once, stand for the state in front of the gang
                                // whichever step finds no level or runs out of registers
                                int more = 0;
                                if constexpr (HELD >= 3) { if (ok && placed < nt) { KFL_STEP(C, KFL_HOLD2); more = 1; } }
                                if (!ok) { cnt = cnt_s; nz = nz_s; extra += placed; fail2 |= 1ull << jj; }  // Statement.Rollback: it booked the tasks it placed and the one that found no node
                                else if (placed < nt) {  // one step more than the lanes hold: the run ends in front of this gang, which then goes the long way from the start (no outcome here: it counts as predicted right and is taken out of `walked` below)
                                    cnt = cnt_s; nz = nz_s; longm |= 1ull << jj; rest = hot | held | (1ull << jj); hot = 0; held = 0; ok = pred;
                                } else { twor |= 1ull << jj; if constexpr (HELD >= 3) nx = kw::writelane(nx, more, jj); }
                                w = (w & ~(1u << 30)) | ((uint32_t)(pred ^ ok) << 30);
                            }
                            if ((w >> 30) & 1) { hot = 0; held = 0; }  // a job that ends differently from its prediction is the round's last: nothing behind it is walked
                            else {
                                if (nz != nz_tab) { KFL_TABLE(); }
                                hot |= held; KFL_CUT(hot);
                            }
                        }
                        KFL_T(2);
                    } while (hot);
                    mismatch |= (int)((w >> 30) & 1);
                    const uint64_t okw = kw::ballot(((c0 >> 29) & 1) != 0) & ~fail2;  // the walked jobs that found room: the first step's word says so, unless a second step was rolled back
                    const uint64_t walked = run0 & ((2ull << jj) - 1) & ~rest, okr = walked & okw;  // (the jobs of the run up to the last one walked)
                    failm |= walked & ~okw; hot |= rest;
                    // the flush: lane j stores the commands of job j
                    okm |= okr;
                    if (mismatch) last_jj = 63 - __builtin_clzll(walked);
                    if (okr) {
                        const int n_my = (int)((okr >> lane) & 1ull) + (int)((twor >> lane) & 1ull) + (HELD >= 3 ? nx : 0);  // 1 .. HELD commands (nx != 0 only in a lane of twor)
                        const int incl = kw::wave_scan_add(n_my), n_run = kw::bcast(incl, 63);
                        KFL_ROOM(n_run);
                        const int pos = wp + incl - n_my;
                        const uint32_t jb = (uint32_t)lane << KFL_JOB_SHIFT;
                        if (n_my >= 1) L.ring[pos & (KFL_RING - 1)] = (uint64_t)(((uint32_t)c0 & 0x7fffffu) | jb) | ((uint64_t)(uint32_t)s.first << 32);
                        int tb_n = s.first + ((c0 >> 12) & 0x7ff) * ((c0 >> 8) & 15);  // a command's task base: the one before it plus k·per of the held word before it
                        if (n_my >= 2) L.ring[(pos + 1) & (KFL_RING - 1)] = (uint64_t)((uint32_t)c1 | jb) | ((uint64_t)(uint32_t)tb_n << 32);
                        if constexpr (HELD >= 3) { tb_n += ((c1 >> 12) & 0x7ff) * ((c1 >> 8) & 15); if (n_my >= 3) L.ring[(pos + 2) & (KFL_RING - 1)] = (uint64_t)((uint32_t)c2 | jb) | ((uint64_t)(uint32_t)tb_n << 32); }
                        wp += n_run;
                        kw::lds_store_rel(&L.head, wp); pub = wp;
                    }
                    KFL_T(3);
                }
                todo |= hot;
                if (mismatch) break;
                if (!hot && lm) {
                    // the long way: a gang of several classes task by task, a gang of one class with more tasks than the stretch reserved room for (or none)
                    const int jj = __builtin_ctzll(todo); todo &= todo - 1;
                    const int pack = kw::bcast(my_pack, jj), first = kw::bcast(s.first, jj);
                    const uint32_t tq = kw::bcast(my_tq, jj);
                    const int flag = pack & 3, qc = (pack >> 2) & 31, nt = (pack >> 7) & 0x7ff;
                    const uint64_t jbits = (uint64_t)((uint32_t)jj << KFL_JOB_SHIFT);
                    KFL_T(1);
                    const int cnt_s = cnt, wp_s = wp; const uint32_t nz_s = nz;
                    int placed = 0, ok = 1;
                    KFL_ROOM(nt);
                    if (!qc) {
                        for (int tb = 0; tb < nt && ok; tb += 64) {
                            const int my_cls = tb + lane < nt ? b.t_cls[first + tb + lane] : 0;
                            const int tc = nt - tb < 64 ? nt - tb : 64;
                            for (int ti = 0; ti < tc; ti++) {
                                const int q1 = kw::bcast(qk, kw::bcast(my_cls, ti));
                                const int g = q1 <= 31 ? KFL_LEVEL_FOR(q1) : 0;
                                if (!g) { ok = 0; break; }
                                KFL_EMIT(g, g - q1, 1, 1, first + placed);
                                KFL_EVENT(g, g - q1, 1, kw::bcast(cnt, g));
                                placed++;
                            }
                        }
                    } else while ((placed < nt) & (ok != 0)) { KFL_STEP(L, KFL_EMIT_RING); }
                    const int fail = ok ^ 1;
                    KFL_T(2);
                    KFL_GANG_END();
                    if (wp - pub >= 64) { kw::lds_store_rel(&L.head, wp); pub = wp; }
                    KFL_T(3);
                    if (g_mis) break;
                }
            }
            if (mismatch) { n_done = base + last_jj + 1; n_out = last_jj + 1; attempted -= jn - n_out; }
            KFL_T(3);
            {   // the stretch's outcomes: what every job ended with, its Statement number and the offset of its operations among the round's (a ballot and a prefix sum)
                const uint64_t outm = n_out >= 64 ? ~0ull : (1ull << n_out) - 1;
                const int nfail = __builtin_popcountll(s.defm & outm) + __builtin_popcountll(failm);  // dead for good (the capacities at their turns: the bookkeeper's part) or walked without room
                decisions += nfail + extra; rollbacks += 2 * nfail;
                const bool my_ok = (okm >> lane) & 1ull;
                const int myv = my_ok ? s.nt : 0, incl = kw::wave_scan_add(myv);
                const int my_stmt = committed + rp.stmt0 + __builtin_popcountll(okm & ((1ull << lane) - 1)), my_opoff = ops + rp.ops0 + incl - myv;
                if (lane < n_out) { b.g_out[base + lane] = (uint8_t)(my_ok ? BF_OK : BF_DEAD); b.g_opoff[base + lane] = my_opoff; b.g_stmt[base + lane] = my_stmt; }
                committed += __builtin_popcountll(okm); ops += kw::bcast(incl, 63); decisions += kw::bcast(incl, 63);  // every task of a committed gang was a decision
            }
            if (wp != pub) { kw::lds_store_rel(&L.head, wp); pub = wp; }
            KFL_T(4);
        }
        #undef KFL_LEVEL_FOR
        #undef KFL_ROOM
        #undef KFL_EMIT
        #undef KFL_EVENT
        #undef KFL_STEP
        #undef KFL_EMIT_RING
        #undef KFL_LOW
        #undef KFL_TABLE
        #undef KFL_CUT
        #undef KFL_HOLD1
        #undef KFL_HOLD2
        #undef KFL_GANG_END
        if (lane == 0) L.fin = n_done;
        kw::lds_store_rel(&L.head, wp);
        kw::lds_store_rel(&L.done, 1);
        const uint64_t dead = kw::ballot(act && (qk > 32 || ((nz >> 1) >> (qk - 1)) == 0));
        if (lane == 0) {
            FillStatus s; s.n_done = n_done; s.mismatch = mismatch; s.all_dead = (C > 0 && dead == (C >= 64 ? ~0ull : ((1ull << C) - 1))) ? 1 : 0; s.planned = V; s.floor_stop = 0; s.pad = 0;
            s.decisions = decisions; s.attempted = attempted; s.committed = committed; s.rollbacks = rollbacks; s.ops = ops; s.dead_mask = dead;  // (decisions: the bookkeeper's part is added below)
            s.cycles_total = kw::clock() - tstart; s.cycles_load = a_wait; s.cycles_update = 0; s.cycles_rescan = 0; s.block_loads = 0;  // (cycles_update / cycles_rescan / block_loads / rescans1: the workers' clocks, added below)
            s.rescans1 = 0; s.rescans2 = wp - n_mark; s.rescans3 = 0;  // rescans2: commands (a command moves the first k nodes of a level; the markers are none)
#ifdef KFL_PROF
            s.cycles_load = pc[0]; s.cycles_update = pc[1]; s.cycles_rescan = pc[2]; s.block_loads = pc[3]; s.rescans1 = pc[4];  // stretch prologue / decode / the gang / its tail / stretch epilogue
#endif
            b.fs[0] = s; b.dead_mask[0] = dead;
        }
    } else if (wave <= v.LV) {
        // ------------------------------------------------------------------ wavefront G = 1 .. LV: the worker of level G.  Everything here is uniform over the wavefront.
        // Under bin-pack the body exists twice: LOW is wavefront 1's, the lowest level's.  Its nodes leave for no level (g2 < g = 1), so its removals form no hand-over entry,
        // look at no pair counter and store nothing for one — a compile-time fact there.  (Under spread the lowest level is a source only when it is the highest non-empty
        // one, and no run of insertions finds its source ahead — a spread command brings a node per word it spans, the targets wait for the sources: DESIGN.md 5.2d — so the
        // spread instantiation keeps ONE body, without runs.)
        constexpr bool RUNS = !SP && KFL_RUN_MIN <= 64;
        auto worker = [&](auto low_) {
        constexpr bool LOW = decltype(low_)::value;
        const int G = LOW ? 1 : wave, lw = (G - 1) * v.NW, l1 = (G - 1) * v.NW1;
        KW_LDS_PTR(uint64_t) dm = (KW_LDS_PTR(uint64_t))&L.dummy[0];
        // the level's first summary in registers: lane j holds the word of group j (bit i: word 64 j + i holds a node; NW1 <= 64).  Only this worker reads and writes it and nobody
        // wants it back, so after this load the s1 region of the LDS is not touched again: "the word is empty now" and "the word was empty" are lane writes.
        uint64_t s1v = lane < v.NW1 ? v.s1[l1 + lane] : 0;
        uint64_t s2 = kw::ballot(s1v != 0);  // second summary: bit j = the 64 words of group j hold a node
        int firstn = KB_INF, cw = -1; uint64_t curw = 0;  // the level's first node (lowest name rank), the word that holds it (index and current value)
        // the first node of the level from the summaries: one lane read, one LDS read
        auto refill = [&]() { if (!s2) { firstn = KB_INF; cw = -1; curw = 0; return; } const int w1 = __builtin_ctzll(s2); cw = w1 * 64 + __builtin_ctzll(kw::bcast(s1v, w1)); curw = kfl_read(&v.gw[lw + cw]); firstn = (cw << 6) + __builtin_ctzll(curw); };
        refill();
        // lane t: this worker's hand-over ring to level t + 1 — entries written, the consumer's progress as last read; lane s: its ring from level s + 1 — entries taken
        int xp = 0, xseen = 0, xc = 0;
        int tail = 0; int64_t w_idle = 0; const int64_t w_start = kw::clock();
        int n_runs = 0, n_serial = 0;  // runs of insertions taken in lanes / sent the serial way
#ifdef KFL_PROF
        // the clocks per kind of event (tools/micro/fill_bench.hip -DKFL_PROF): cycles and events, kept by lane 0 in the LDS; the product build carries none of it
        int64_t wt = kw::clock();
        #define KFL_WT0() (wt = kw::clock())
        #define KFL_WK(kind_) do { const int64_t n_ = kw::clock(); if (lane == 0) { L.wk_cyc[G - 1][kind_] += n_ - wt; L.wk_cnt[G - 1][kind_]++; } wt = n_; } while (0)
#else
        #define KFL_WT0() (void)0
        #define KFL_WK(kind_) (void)0
#endif
        for (;;) {
            const int head = kfl_load(&L.head);
            if (tail == head) {
                if (kfl_load(&L.done) && tail == kfl_load(&L.head)) break;
                const int64_t i0 = kw::clock(); while (kfl_load(&L.head) == tail && !kfl_load(&L.done)) kw::relax(); w_idle += kw::clock() - i0;
                continue;
            }
            while (tail < head) {
                // a batch of up to 64 commands, one per lane: the ones that name this level are walked, the others cost nothing
                const int nb = head - tail < 64 ? head - tail : 64;
                const uint64_t mc = L.ring[(tail + lane) & (KFL_RING - 1)];  // (lanes beyond the batch read a slot that is not used)
                uint64_t mine = kw::ballot(lane < nb && ((int)(mc & 15) == G || (int)((mc >> 4) & 15) == G));
                // runb: the insertions of `mine` whose predecessor in `mine` is an insertion too — the carry of (its insertions << 1) through the commands that are not this
                // level's lands on the next one that is.  (The top level takes nothing in: the word stays 0 there.)
                uint64_t runb = 0;
                if (RUNS) { const uint64_t tg = kw::ballot(lane < nb && (int)((mc >> 4) & 15) == G); runb = (~mine + (tg << 1)) & mine & tg; }
                while (mine) {
                    KFL_WT0();
                    const int ci = __builtin_ctzll(mine); mine &= mine - 1;
                    const int ca = kw::bcast((int)(uint32_t)mc, ci);
                    const int g = ca & 15, g2 = (ca >> 4) & 15;
                    if (g == G) {
                        // SOURCE: the level's first k nodes leave it, `per` tasks on each.  Every LDS store goes through a pointer that is lane 0's target or the lane's own dummy slot.
                        const int per = (ca >> 8) & 15; int left = (ca >> 12) & 0x7ff, tb = kw::bcast((int)(uint32_t)(mc >> 32), ci);
                        const int pr = g2 >= 1 ? kfl_pair(G, g2) : KFL_PAIRS;  // (no level: the ring nobody reads)
                        const int xl = (g2 - 1) & 63;                          // (no level: lane 63, which is never counted up)
                        const bool hand = !LOW && (SP || g2 >= 1);  // (the lowest level hands nothing over.  The other levels branch round the entry of a node that leaves for no level — one uniform branch against fifteen instructions and three stores: the replay has it 50 cycles a removal cheaper under bin-pack; under spread, where few nodes leave for no level, the ring nobody reads is cheaper)
#ifdef KFL_PROF
                        const int k_all = left; int n_words = 0, n_emptied = 0;
#endif
                        if (__builtin_expect(left == 1, 1)) {
                            // the usual command, straight through: ONE node, the level's first, leaves with `per` tasks on it; the word it sat in stays non-empty and the hand-over ring has
                            // room (either of the two failing: one rarely taken exit each).  The replay has this path at 435 cycles against 806 through the ballot below (profiles/r12).
                            const int w = cw; const uint64_t mask = curw & (0 - curw), neww = curw ^ mask;
                            b.t_node[tb + (lane < per ? lane : per - 1)] = firstn;  // (its tasks all sit on it, per <= 8; the lanes beyond them store the last one's again: no branch)
                            kfl_write(&v.gw[lw + w], neww, dm);
                            if (hand) {
                                const int n_w = kw::bcast(xp, xl);
                                if (__builtin_expect(n_w - kw::bcast(xseen, xl) >= KFL_XR, 0)) { int t; while (n_w - (t = kfl_load(&L.xtail[pr])) >= KFL_XR) kw::relax(); if (lane == xl) xseen = t; }
                                KW_LDS_PTR(FlMove) e = lane == 0 ? (KW_LDS_PTR(FlMove))&L.x[pr][n_w & (KFL_XR - 1)] : (KW_LDS_PTR(FlMove))&L.xdummy[lane];
                                e->mask = mask; e->w = w | (1 << 30);
                                kw::lds_store_ordered((int32_t*)&e->seq, n_w + 1);
                                xp += lane == g2 - 1 ? 1 : 0;
                            }
                            if (__builtin_expect(neww != 0, 1)) { curw = neww; firstn = (w << 6) + __builtin_ctzll(neww); }
                            else {
                                const int w1 = w >> 6; const uint64_t m1 = kw::bcast(s1v, w1) & ~(1ull << (w & 63));
                                s1v = kw::writelane(s1v, m1, w1);
                                s2 &= ~((uint64_t)(uint32_t)(1 - kw::nonzero01((uint32_t)m1 | (uint32_t)(m1 >> 32))) << w1);
                                refill();
#ifdef KFL_PROF
                                n_emptied++;
#endif
                            }
                            left = 0;
                        }
                        while (__builtin_expect(left > 0, 0)) {
                            // several nodes, word by word, each word straight through: the first m = min(nodes left, nodes of the cached word) nodes of the word that holds the level's
                            // first node are picked by ONE ballot (lane i ranks bit i of the word), the lanes that hold them write their tasks' nodes, and (word, mask) is handed over in
                            // one entry.  No loop over the nodes, none over the bits; a command whose nodes span words comes round again for the next word.
                            const int w = cw; const uint64_t word = curw;
                            const int pop = __builtin_popcountll(word), m = left < pop ? left : pop;
                            const int r = kw::rank_below(word);
                            const bool sel = ((word >> lane) & 1ull) != 0 && r < m;
                            const uint64_t mask = kw::ballot(sel), neww = word ^ mask;
                            // the tasks' nodes, unpredicated: the lane of the node of rank r stores it for the tasks r·per .. r·per + per − 1 (a uniform loop over per <= 8), every other
                            // lane stores the word's last node for its last task again.  One node: its tasks' lanes store it (lanes < per; the lanes beyond them the last one's again).
                            const int one = m == 1, lastn = (w << 6) + 63 - __builtin_clzll(mask);
                            const int val = sel ? (w << 6) + lane : lastn;
                            const int onem = 0 - one, off1 = lane < per ? lane : per - 1, offm = sel ? r * per : m * per - 1;  // (selected by masks: no branch on `one`)
                            int a = tb + ((off1 & onem) | (offm & ~onem));
                            b.t_node[a] = val;
                            if (__builtin_expect((per & ~onem) > 1, 0)) {  // several nodes with several tasks each: the tasks behind a node's first
                                const int stp = sel ? 1 : 0;
                                _Pragma("nounroll") for (int j = 1; j < per; j++) { a += stp; b.t_node[a] = val; }
                            }
                            kfl_write(&v.gw[lw + w], neww, dm);
                            left -= m; tb += m * per;
                            // one entry for the target level's worker
                            if (hand) {
                                const int n_w = kw::bcast(xp, xl);
                                if (__builtin_expect(n_w - kw::bcast(xseen, xl) >= KFL_XR, 0)) { int t; while (n_w - (t = kfl_load(&L.xtail[pr])) >= KFL_XR) kw::relax(); if (lane == xl) xseen = t; }
                                KW_LDS_PTR(FlMove) e = lane == 0 ? (KW_LDS_PTR(FlMove))&L.x[pr][n_w & (KFL_XR - 1)] : (KW_LDS_PTR(FlMove))&L.xdummy[lane];
                                e->mask = mask; e->w = w | (left == 0 ? 1 << 30 : 0);
                                kw::lds_store_ordered((int32_t*)&e->seq, n_w + 1);
                                xp += lane == g2 - 1 ? 1 : 0;
                            }
                            if (__builtin_expect(neww != 0, 1)) { curw = neww; firstn = (w << 6) + __builtin_ctzll(neww); }
                            else {  // the word is empty: its bit in the first summary goes (a lane write), and the level's first node is the first node of the next word
                                const int w1 = w >> 6; const uint64_t m1 = kw::bcast(s1v, w1) & ~(1ull << (w & 63));
                                s1v = kw::writelane(s1v, m1, w1);
                                s2 &= ~((uint64_t)(uint32_t)(1 - kw::nonzero01((uint32_t)m1 | (uint32_t)(m1 >> 32))) << w1);  // (the group's bit goes with its last word — as a number, not as a comparison)
                                refill();
#ifdef KFL_PROF
                                n_emptied++;
#endif
                            }
#ifdef KFL_PROF
                            n_words++;
#endif
                        }
#ifdef KFL_PROF
                        if (k_all == 1) { if (n_emptied) KFL_WK(1); else KFL_WK(0); } else if (n_words == 1) KFL_WK(2); else KFL_WK(3);
#endif
                    } else {
                        // TARGET: take the command's nodes in as the source level's worker hands them over
                        const int pr = kfl_pair(g, G);
                        if (RUNS && (runb & mine & (0 - mine)) != 0) {
                            // A RUN OF INSERTIONS: the next command of `mine` brings nodes too.  Between two removals insertions commute — they or bits into words, set summary
                            // bits and lower the first node —, so the insertions from this command's source level in front of the next other command of `mine` (a removal, or an
                            // insertion from another level: that one starts a run of its own), KFL_RUN_MIN or more of them and at most 16 command slots on, are taken in ONE pass:
                            // lane i reads the i-th entry of the pair's ring behind the ones taken (the ring is KFL_XR = 32 entries: lanes 32-63 read what lanes 0-31 read and take
                            // no part), every entry lane ors its mask into its word, a uniform loop of a few scalar instructions per entry tells the first summary and finds the
                            // first node, the ring moves on once.  Nothing here waits: if the source has not yet handed over all the run needs, nothing has been consumed and
                            // the run goes entry by entry, which waits as it always did.
                            const uint64_t stop = mine & ~runb;
                            uint64_t run = mine & (stop ? (stop & (0 - stop)) - 1 : ~0ull) & (0xffffull << ci);
                            const uint64_t other = kw::ballot((int)(mc & 15) != g) & run;
                            run &= other ? (other & (0 - other)) - 1 : ~0ull;
                            const int cA = 1 + __builtin_popcountll(run);  // commands of the run
                            if (cA >= KFL_RUN_MIN) {
                                const int nr = kw::bcast(xc, g - 1), en = nr + (lane & (KFL_XR - 1)), sl = en & (KFL_XR - 1);
                                // sequence number first, the entry behind it in the same trip
                                const int sq = kw::lds_load_ordered(&L.x[pr][sl].seq), wf_v = kw::lds_load_relaxed(&L.x[pr][sl].w); const uint64_t mk_v = kw::lds_load_relaxed(&L.x[pr][sl].mask);
                                const uint32_t vm = (uint32_t)kw::ballot(sq == en + 1), lm = (uint32_t)kw::ballot(sq == en + 1 && ((wf_v >> 30) & 1) != 0);
                                // the run's entries: the valid prefix of the ring up to the cA-th `last` flag (a command of several entries needs no special case); 0: not all there
                                int n = 0;
                                const uint32_t all = (uint32_t)((1ull << cA) - 1);
                                if (__builtin_expect((lm & all) == all, 1)) n = cA;  // (the usual run: every command brought one entry)
                                else {
                                    uint32_t m = lm & (uint32_t)((1ull << __builtin_ctzll(~(uint64_t)vm)) - 1);
                                    if (__builtin_popcount(m) >= cA) { for (int j = 1; j < cA; j++) m &= m - 1; n = __builtin_ctz(m) + 1; }
                                }
                                if (__builtin_expect(n != 0, 1)) {
                                    mine &= ~run; n_runs++;
                                    {   // the masks into their words: an LDS `or` that returns nothing; lanes without an entry or into their dummy slot, two entries of one word are the LDS's business
                                        KW_LDS_PTR(uint64_t) q = lane < n ? (KW_LDS_PTR(uint64_t))&v.gw[lw + (wf_v & 0x3fffffff)] : dm + lane;
                                        kw::lds_or(q, mk_v);
                                    }
                                    // the ring moves on, behind the reads, once: a producer that waits for room is released now
                                    kw::lds_store_ordered(&L.xtail[pr], nr + n);
                                    xc += lane == g - 1 ? n : 0;
                                    // entry by entry on the scalar unit: the word's bit in the first summary; the level's first node = the lowest of today's and the entries' — its word
                                    // is the cached one, which takes the run's masks for it, or lies below it and was empty before the run (a non-empty word other than the cached one
                                    // lies above it: tests/test_fill_levels_workers.py — for the run as a whole), so its value is the or of the run's masks for it
                                    int minw = cw >= 0 ? cw : 0x7fffffff; uint64_t acc = curw;
                                    for (int el = 0; el < n; el++) {
                                        const int w = kw::bcast(wf_v, el) & 0x3fffffff, w1 = w >> 6; const uint64_t mask = kw::bcast(mk_v, el);
                                        s1v = kw::writelane(s1v, kw::bcast(s1v, w1) | (1ull << (w & 63)), w1);
                                        acc = w < minw ? mask : w == minw ? acc | mask : acc; minw = w < minw ? w : minw;
                                    }
                                    s2 = kw::ballot(s1v != 0);
                                    cw = minw; curw = acc; firstn = (cw << 6) + __builtin_ctzll(curw);
#ifdef KFL_PROF
                                    { const int64_t n_ = kw::clock(); if (lane == 0) { L.wk_cyc[G - 1][7] += n_ - wt; L.wk_cnt[G - 1][7]++; L.wk_cnt[G - 1][8] += n; } wt = n_; }
#endif
                                    continue;
                                }
                                runb &= ~run; n_serial++;  // the source is behind: this command and the run's others one by one
                                KFL_WK(9);
                            }
                        }
                        for (bool last = false; !last;) {
                            const int n_r = kw::bcast(xc, g - 1);
                            const int sl = n_r & (KFL_XR - 1);
                            // the sequence number, then the entry behind it, in one trip to the LDS: the LDS serves a wavefront's reads in issue order and the producer stored the number last
                            // (the reads of the entry are atomic ones so that the compiler leaves them in front of the test)
                            int sq = kw::lds_load_ordered(&L.x[pr][sl].seq), wf_v = kw::lds_load_relaxed(&L.x[pr][sl].w); uint64_t mk_v = kw::lds_load_relaxed(&L.x[pr][sl].mask);
                            if (__builtin_expect(kw::uni(sq) != n_r + 1, 0)) { const int64_t i0 = kw::clock(); while (kfl_load(&L.x[pr][sl].seq) != n_r + 1) kw::relax(); w_idle += kw::clock() - i0; wf_v = kw::lds_load_relaxed(&L.x[pr][sl].w); mk_v = kw::lds_load_relaxed(&L.x[pr][sl].mask); KFL_WT0(); }
                            const int wf = kw::bcast(wf_v, 0), w = wf & 0x3fffffff; const uint64_t mask = kw::bcast(mk_v, 0);
                            last = (wf >> 30) & 1;
                            kw::lds_store_ordered(&L.xtail[pr], n_r + 1);
                            if (lane == g - 1) xc++;
                            if (w == cw) { curw |= mask; kfl_write(&v.gw[lw + w], curw, dm); firstn = (w << 6) + __builtin_ctzll(curw); KFL_WK(4); }
                            else {
                                // another word: the bits go in with an LDS `or` that returns nothing (one writer per level: a store that merges), the first summary is told in a lane —
                                // nothing is read.  A node below the level's first one makes its word the cached one; that word was EMPTY (a non-empty word other than the cached one
                                // lies above it, and so does every node of it), so its value is the entry's mask.  An empty level is the same case: every node lies below KB_INF.
                                const int w1 = w >> 6;
#ifdef KFL_PROF
                                const bool was_empty = ((kw::bcast(s1v, w1) >> (w & 63)) & 1ull) == 0;
#endif
                                { KW_LDS_PTR(uint64_t) q = lane == 0 ? (KW_LDS_PTR(uint64_t))&v.gw[lw + w] : dm + lane; kw::lds_or(q, mask); }
                                s1v = kw::writelane(s1v, kw::bcast(s1v, w1) | (1ull << (w & 63)), w1); s2 |= 1ull << w1;
                                const int n = (w << 6) + __builtin_ctzll(mask), fn = kw::uni(firstn);
                                const bool lower = n < fn;
                                firstn = lower ? n : fn; cw = lower ? w : cw; curw = lower ? mask : curw;
#ifdef KFL_PROF
                                if (was_empty) KFL_WK(5); else KFL_WK(6);
#endif
                            }
                        }
                    }
                }
                tail += nb;
            }
            kw::lds_store_rel(&L.tail[G - 1], tail);
        }
        #undef KFL_WT0
        #undef KFL_WK
        if (lane == 0) { L.w_idle[G - 1] = w_idle; L.w_total[G - 1] = kw::clock() - w_start; }
#ifdef KFL_RUN_STATS
        my_runs = (int64_t)n_runs | ((int64_t)n_serial << 32);
#endif
        };
        if constexpr (!SP) { if (wave == 1) worker(std::true_type{}); else worker(std::false_type{}); } else worker(std::false_type{});
    } else if (wave == v.LV + 1) {
        // ------------------------------------------------------------------ wavefront LV + 1: the bookkeeper.  It replays the commands on the capacities (lane q − 1: capq) and books,
        // for every dead-for-good gang, the capacity of its request size at its turn.  A command names its job (bits 23-28); a marker (g = 0) stands in front of every stretch's commands.
        const int qk = lane < C ? (int)c.cls[lane].req[KAI_RES_GPU] : 0x7fffffff;
        const uint32_t tab = kfl_tab(lane, v.LV);
        int capq = 0;
        { const int cnt = lane < v.LV ? L.cnt0[lane] : 0; for (int g = 1; g <= v.LV; g++) capq += kfl_quot(tab, g) * kw::bcast(cnt, g - 1); }
        int dec_v = 0;                     // lane q − 1: Σ of the capacities the dead gangs that ask for q devices met at their turns
        int base = rp.start - 64, seg_lo = 0;   // the stretch the bookkeeper is in (none before the first marker); its jobs below seg_lo are booked
        bool in = false;
        FlStretch s; s.valid = false; s.flag = BF_GATE; s.first = 0; s.nt = 0; s.q = 0; s.is_def = false; s.defm = 0; s.todo = 0;
        uint64_t failm = 0;                // lane q − 1: the stretch's dead-for-good jobs that ask for q devices
        const uint64_t tab4 = (uint64_t)tab << 4;  // the quotients with g as the index: (tab4 >> 4g) & 15, 0 for g = 0
        auto enter = [&]() {
            const int gi = base + lane; s.valid = gi < V; const int gc = s.valid ? gi : (V > 0 ? V - 1 : 0);
            s.flag = s.valid ? (int)b.g_flag[gc] : (int)BF_GATE; s.nt = s.valid ? b.g_nt[gc] : 0;
            kfl_classify(s, s.valid ? b.g_ucls[gc] : 0, qk, capq);
            failm = 0; if (s.defm) for (int q = 1; q <= v.LV; q++) { const uint64_t m = kw::ballot(s.is_def && s.q == q); if (lane == q - 1) failm = m; }
            seg_lo = 0; in = true;
        };
        // the dead-for-good jobs [seg_lo, hi) of the stretch book their decisions with the capacities as they are now
        auto book = [&](int hi) { if (hi > seg_lo) { const uint64_t sm = (hi >= 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << seg_lo) - 1); if (s.defm & sm) dec_v += capq * __builtin_popcountll(failm & sm); seg_lo = hi; } };
        int tail = 0; int64_t w_idle = 0; const int64_t w_start = kw::clock();
        for (;;) {
            const int head = kfl_load(&L.head);
            if (tail == head) {
                if (kfl_load(&L.done) && tail == kfl_load(&L.head)) break;
                const int64_t i0 = kw::clock(); while (kfl_load(&L.head) == tail && !kfl_load(&L.done)) kw::relax(); w_idle += kw::clock() - i0;
                continue;
            }
            while (tail < head) {
                const int nb = head - tail < 64 ? head - tail : 64;
                const uint32_t mc = (uint32_t)L.ring[(tail + lane) & (KFL_RING - 1)];
                for (int ci = 0; ci < nb; ci++) {
                    const uint32_t ca = kw::bcast(mc, ci);
                    const int g = ca & 15, g2 = (ca >> 4) & 15, k = (ca >> 12) & 0x7ff, jj = (ca >> KFL_JOB_SHIFT) & 63;
                    if (__builtin_expect(g == 0, 0)) { if (in) book(64); base += 64; enter(); continue; }  // a marker: the rest of the stretch behind, the next one classified with the capacities as they are now
                    {   // the dead gangs in front of the command's job met the capacities before it (no branch: an empty segment books nothing; jj >= seg_lo, the commands come in the jobs' order)
                        const uint64_t sm = ((1ull << jj) - 1) & ~((1ull << seg_lo) - 1);
                        dec_v += capq * __builtin_popcountll(failm & sm);
                        seg_lo = jj;
                    }
                    capq -= k * ((int)((tab4 >> (4 * g)) & 15) - (int)((tab4 >> (4 * g2)) & 15));
                }
                tail += nb;
            }
            kw::lds_store_rel(&L.tail[KFL_LMAX], tail);
        }
        // the last stretch behind its last command, up to the last job the counting machine executed
        const int fin = kfl_load(&L.fin);
        if (in) book(fin - base < 64 ? fin - base : 64);
        int total = 0; for (int l = 0; l < v.LV; l++) total += kw::bcast(dec_v, l);
        if (lane == 0) { L.b_dec = total; L.w_idle[KFL_LMAX] = w_idle; L.w_total[KFL_LMAX] = kw::clock() - w_start; }
    }
    kw::sync();
#ifdef KFL_RUN_STATS
    if (lane == 0 && my_runs != 0) kw::atomic_add((unsigned long long*)&b.fs[0].rescans3, (unsigned long long)my_runs);  // (the counting machine wrote 0 in front of the barrier)
#endif
    if (tid == 0) {
        b.fs[0].decisions += L.b_dec;
#if defined(KFL_PROF) && defined(__HIPCC__)
        for (int l = 0; l < KFL_LMAX; l++) { for (int k = 0; k < KFL_WKINDS; k++) { kfl_prof_workers[l][k][0] = L.wk_cyc[l][k]; kfl_prof_workers[l][k][1] = L.wk_cnt[l][k]; } kfl_prof_workers[l][KFL_WKINDS][0] = L.w_idle[l]; kfl_prof_workers[l][KFL_WKINDS][1] = L.w_total[l]; }
#endif
#ifndef KFL_PROF
        // the readers' clocks: idle and total summed, the busiest one's busy cycles and its level (9 = the bookkeeper)
        int64_t idle = 0, total = 0, busy = 0; int lvl = 0;
        for (int l = 0; l <= KFL_LMAX; l++) { if (l >= v.LV && l < KFL_LMAX) continue; idle += L.w_idle[l]; total += L.w_total[l]; const int64_t x = L.w_total[l] - L.w_idle[l]; if (x > busy) { busy = x; lvl = l + 1; } }
        b.fs[0].cycles_update = idle; b.fs[0].cycles_rescan = total; b.fs[0].block_loads = busy; b.fs[0].rescans1 = lvl;
#endif
    }
    for (int i = tid; i < v.LV * v.NW; i += T) b.bk_words[i] = v.gw[i];
}

// the entry point picks the instantiation by the session's strategy on the GPU (the emulator's launchers call it; the device launches one of the two kernels below)
KW_BODY void kb_fill_levels(const KaiCtx& c, RoundParams rp, BucketParams bp) { if (c.gpu_strategy == KAI_SPREAD) kb_fill_levels_t<1>(c, rp, bp); else kb_fill_levels_t<0>(c, rp, bp); }

#if defined(__HIPCC__)
__global__ void __launch_bounds__(64 * (KFL_LMAX + 2)) k_fill_levels(KaiCtx c, RoundParams rp, BucketParams bp) { kb_fill_levels_t<0>(c, rp, bp); }
__global__ void __launch_bounds__(64 * (KFL_LMAX + 2)) k_fill_levels_spread(KaiCtx c, RoundParams rp, BucketParams bp) { kb_fill_levels_t<1>(c, rp, bp); }
#endif

}  // namespace kai
