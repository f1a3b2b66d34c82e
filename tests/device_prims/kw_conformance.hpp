// kw_conformance.hpp — TEST INFRASTRUCTURE: one kernel body per group of SIMT primitives, written against kai_simt.hpp and the product headers only.  The same text is
// compiled twice: by hipcc for gfx950 (kw_conformance.hip -> libkwconf.so, tests/test_gpu_kw_conformance.py) and by plain g++ on the lock-step emulator
// (kw_conformance_sim.cpp, tests/test_kw_conformance.py).  Both are compared with tests/kw_conformance_cases.py, which states each primitive's contract in numpy and plain Python
// integers.  The bodies call the product's own functions; nothing is restated here.  Included behind the product headers (the including file chooses them).
//
// Buffers are flat arrays of 64-bit words, one record per thread at index (workgroup * workgroup size + thread) unless a body says otherwise; doubles travel as their bits,
// ints sign-extended.  `nw` is the number of input words.  Every body has a bounded trip count and waits for nothing but kw::sync().
#pragma once
#include <stdint.h>

namespace kwc {
using namespace kai;

KW_BODY int gidx() { return kw::bid() * kw::bdim() + kw::tid(); }
KW_BODY double f64_of(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
KW_BODY uint64_t bits_of(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
KW_BODY uint64_t word_of(int v) { return (uint64_t)(int64_t)v; }
KW_BODY PlanKey key_at(const uint64_t* p) { PlanKey k; k.w0 = p[0]; k.w1 = p[1]; k.w2 = p[2]; k.w3 = p[3]; return k; }
KW_BODY void key_to(uint64_t* p, const PlanKey& k) { p[0] = k.w0; p[1] = k.w1; p[2] = k.w2; p[3] = k.w3; }

// in: v                                    out: wave_scan_add<int>(v)
KW_BODY void scan_int(const uint64_t* in, uint64_t* out, int64_t) { const int g = gidx(); out[g] = word_of(kw::wave_scan_add<int>((int)in[g])); }
// in: bits of v                            out: bits of wave_scan_add<double>(v)
KW_BODY void scan_f64(const uint64_t* in, uint64_t* out, int64_t) { const int g = gidx(); out[g] = bits_of(kw::wave_scan_add<double>(f64_of(in[g]))); }
// in: key, n                               out: kw::wave_max_u64(key); key, n of kw::wave_argmax_first; key, n of kai::wave_argmax_first (the device's own; the emulator has the one)
KW_BODY void wave_max(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(); const uint64_t key = in[2 * g]; const int n = (int)in[2 * g + 1];
    out[5 * g] = kw::wave_max_u64(key);
    uint64_t k1 = key; int n1 = n; kw::wave_argmax_first(k1, n1);
    out[5 * g + 1] = k1; out[5 * g + 2] = word_of(n1);
#if defined(__HIPCC__)
    unsigned long long k2 = key; int n2 = n; kai::wave_argmax_first(k2, n2);
    out[5 * g + 3] = k2; out[5 * g + 4] = word_of(n2);
#else
    out[5 * g + 3] = k1; out[5 * g + 4] = word_of(n1);
#endif
}
// in: w0 w1 w2 w3 valid have_carry c0 c1 c2 c3          out: the four words of kb_wave_scan_max
KW_BODY void key_scan(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(); const uint64_t* r = in + 10 * g;
    key_to(out + 4 * g, kb_wave_scan_max(key_at(r), r[4] != 0, key_at(r + 6), r[5] != 0));
}
// in: NV doubles                           out: incl[NV] total[NV] of a first call; incl[NV] total[NV] of a second one on twice the values, thread 0 adding the first call's totals to its own
// (the carry of the next step, as k_plan_scan's loop has it).  The second call writes PlanScanLds right behind the first call's reads: the barrier between them is under test.
template <int NV> KW_BODY void block_add(const uint64_t* in, uint64_t* out, int64_t) {
    KW_SHARED PlanScanLds L;
    const int g = gidx(); double d[NV], i1[NV], t1[NV], i2[NV], t2[NV];
    for (int k = 0; k < NV; k++) d[k] = f64_of(in[NV * g + k]);
    kb_block_scan_add<NV>(L, d, i1, t1);
    for (int k = 0; k < NV; k++) d[k] = kw::tid() == 0 ? d[k] + t1[k] : d[k] + d[k];  // (every wavefront's total differs from the first call's: a total read late is seen)
    kb_block_scan_add<NV>(L, d, i2, t2);
    uint64_t* o = out + 4 * NV * g;
    for (int k = 0; k < NV; k++) { o[k] = bits_of(i1[k]); o[NV + k] = bits_of(t1[k]); o[2 * NV + k] = bits_of(i2[k]); o[3 * NV + k] = bits_of(t2[k]); }
}
KW_BODY void block_add3(const uint64_t* in, uint64_t* out, int64_t nw) { block_add<3>(in, out, nw); }
KW_BODY void block_add6(const uint64_t* in, uint64_t* out, int64_t nw) { block_add<6>(in, out, nw); }
// in: a0..a3 va  b0..b3 vb  have_carry c0..c3  have2     out: key, last of kb_block_scan_max(a, carry); key, last of kb_block_scan_max(b, carry = the first call's last)
// have2 (is the first call's `last` a key: a carry, or any valid a in the workgroup) comes with the input: the function does not return it
KW_BODY void block_max(const uint64_t* in, uint64_t* out, int64_t) {
    KW_SHARED PlanScanLds L;
    const int g = gidx(); const uint64_t* r = in + 16 * g; uint64_t* o = out + 16 * g;
    PlanKey l1, l2;
    const PlanKey o1 = kb_block_scan_max(L, key_at(r), r[4] != 0, key_at(r + 11), r[10] != 0, l1);
    const PlanKey o2 = kb_block_scan_max(L, key_at(r + 5), r[9] != 0, l1, r[15] != 0, l2);
    key_to(o, o1); key_to(o + 4, l1); key_to(o + 8, o2); key_to(o + 12, l2);
}
// in: as block_max (have2 unused)          out: pre[4] have_pre last[4] have_last of kb_block_excl_max(a, carry); the same of (b, carry = the first call's last / have_last)
KW_BODY void block_excl(const uint64_t* in, uint64_t* out, int64_t) {
    KW_SHARED PlanScanLds L;
    const int g = gidx(); const uint64_t* r = in + 16 * g; uint64_t* o = out + 20 * g;
    PlanKey p1, l1, p2, l2; bool hp1, hl1, hp2, hl2;
    kb_block_excl_max(L, key_at(r), r[4] != 0, key_at(r + 11), r[10] != 0, p1, hp1, l1, hl1);
    kb_block_excl_max(L, key_at(r + 5), r[9] != 0, l1, hl1, p2, hp2, l2, hl2);
    key_to(o, p1); o[4] = hp1; key_to(o + 5, l1); o[9] = hl1; key_to(o + 10, p2); o[14] = hp2; key_to(o + 15, l2); o[19] = hl2;
}
// in: v1 v2                                out: incl, total of sg_wg_scan(v1); incl, total of sg_wg_scan(v2) — two calls in a row on one s_w
KW_BODY void wg_scan(const uint64_t* in, uint64_t* out, int64_t) {
    KW_SHARED int32_t s_w[64];
    const int g = gidx(); int t1 = 0, t2 = 0;
    const int i1 = sg_wg_scan((int)in[2 * g], s_w, t1), i2 = sg_wg_scan((int)in[2 * g + 1], s_w, t2);
    out[4 * g] = word_of(i1); out[4 * g + 1] = word_of(t1); out[4 * g + 2] = word_of(i2); out[4 * g + 3] = word_of(t2);
}
// kb_plan_setup itself, one workgroup, on a context of M = Q + 1 queue nodes of height 0 (no pass over the heights: n_h = 1).  32-bit words.
// in: Q h_leaf  q_child_off[M + 1]  lq_cur[M]  lq_end[M]  h_nodes[M]
// out: q_ebase[M] q_kbase[M] q_cnt[M] q_sent[M] q_valid[M] q_nk[M] q_taken[M] plan_tot[2] q_complete[M bytes]
KW_BODY void plan_setup(const uint64_t* in64, uint64_t* out64, int64_t) {
    int32_t* in = const_cast<int32_t*>(reinterpret_cast<const int32_t*>(in64)); int32_t* out = reinterpret_cast<int32_t*>(out64);
    const int M = in[0] + 1;
    KaiCtx c{}; RoundParams rp{}; rp.h_leaf = in[1];
    c.Q = in[0]; c.q_child_off = (KAI_GP(const int32_t))(in + 2); c.lq_cur = (KAI_GP(int32_t))(in + 3 + M); c.lq_end = (KAI_GP(int32_t))(in + 3 + 2 * M);
    c.bt.n_h = 1; c.bt.dev_loop = 0; c.bt.h_nodes = (KAI_GP(int32_t))(in + 3 + 3 * M);
    c.bt.q_ebase = (KAI_GP(int32_t))out; c.bt.q_kbase = (KAI_GP(int32_t))(out + M); c.bt.q_cnt = (KAI_GP(int32_t))(out + 2 * M); c.bt.q_sent = (KAI_GP(int32_t))(out + 3 * M);
    c.bt.q_valid = (KAI_GP(int32_t))(out + 4 * M); c.bt.q_nk = (KAI_GP(int32_t))(out + 5 * M); c.bt.q_taken = (KAI_GP(int32_t))(out + 6 * M); c.bt.plan_tot = (KAI_GP(int32_t))(out + 7 * M);
    c.bt.q_complete = (KAI_GP(uint8_t))(out + 7 * M + 2);
    kb_plan_setup(c, rp);
}
// in: v, u (the same in every lane of a wavefront), src (likewise)
// out: bcast of (int)v, (uint32_t)(v >> 32), v, v as a double; uni of (int)u, (uint32_t)(u >> 32), u; writelane((int)v, (int)u, src), writelane(v, u, src); opaque(u), opaque((uint32_t)u)
KW_BODY void lane_ops(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(); const uint64_t v = in[3 * g], u = in[3 * g + 1]; const int src = (int)in[3 * g + 2]; uint64_t* o = out + 11 * g;
    o[0] = word_of(kw::bcast((int)v, src)); o[1] = kw::bcast((uint32_t)(v >> 32), src); o[2] = kw::bcast(v, src); o[3] = bits_of(kw::bcast(f64_of(v), src));
    o[4] = word_of(kw::uni((int)u)); o[5] = kw::uni((uint32_t)(u >> 32)); o[6] = kw::uni(u);
    o[7] = word_of(kw::writelane((int)v, (int)u, src)); o[8] = kw::writelane(v, u, src);
    o[9] = kw::opaque(u); o[10] = kw::opaque((uint32_t)u);
}
// in: v, src (per lane: a live lane of the wavefront)
// out: shfl of (int)v, v as a double, v, (int64_t)v from src; shfl_up of (int)v by 1 2 4 8 16 32 63; shfl_up of v by the same
KW_BODY void shfl(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(); const uint64_t v = in[2 * g]; const int src = (int)in[2 * g + 1]; uint64_t* o = out + 18 * g;
    o[0] = word_of(kw::shfl((int)v, src)); o[1] = bits_of(kw::shfl(f64_of(v), src)); o[2] = kw::shfl(v, src); o[3] = (uint64_t)kw::shfl((int64_t)v, src);
    const int ds[7] = {1, 2, 4, 8, 16, 32, 63};
    for (int i = 0; i < 7; i++) { o[4 + i] = word_of(kw::shfl_up((int)v, ds[i])); o[11 + i] = kw::shfl_up(v, ds[i]); }
}
// in: p, m (the same in every lane of a wavefront)       out: ballot(p != 0), rank_below(m)
KW_BODY void ballot_rank(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx();
    out[2 * g] = kw::ballot(in[2 * g] != 0); out[2 * g + 1] = word_of(kw::rank_below(kw::uni(in[2 * g + 1])));
}
// in: v, bit (both the same in every lane of a wavefront)        out: nonzero01((uint32_t)v), bit_clear((uint32_t)v, bit), bit_set((uint32_t)v, bit), bit_clear(v, bit)
KW_BODY void scalar_bits(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(); const uint64_t v = kw::uni(in[2 * g]); const int bit = kw::uni((int)in[2 * g + 1]); uint64_t* o = out + 4 * g;
    o[0] = word_of(kw::nonzero01((uint32_t)v)); o[1] = kw::bit_clear((uint32_t)v, bit); o[2] = kw::bit_set((uint32_t)v, bit); o[3] = kw::bit_clear(v, bit);
}
// in: a b c v
// out: the lane's own LDS word starts as a: lds_xor(b) -> old; lds_or(c); lds_xor(a) -> old; the word at the end.  Then kfl_write(word of the wavefront, v, dummy area) and
// kfl_read(word): what every lane read; the word; the lane's slot of the 64-entry dummy area (both start as ~0)
KW_BODY void lds_ops(const uint64_t* in, uint64_t* out, int64_t) {
    KW_SHARED uint64_t s_own[1024]; KW_SHARED uint64_t s_word[16]; KW_SHARED uint64_t s_dummy[16 * 64];
    const int g = gidx(), t = kw::tid(), w = t >> 6; const uint64_t* r = in + 4 * g; uint64_t* o = out + 6 * g;
    KW_LDS_PTR(uint64_t) p = (KW_LDS_PTR(uint64_t))&s_own[t];
    *p = r[0];
    o[0] = kw::lds_xor(p, r[1]); kw::lds_or(p, r[2]); o[1] = kw::lds_xor(p, r[0]); o[2] = *p;
    KW_LDS_PTR(uint64_t) word = (KW_LDS_PTR(uint64_t))&s_word[w]; KW_LDS_PTR(uint64_t) dummy = (KW_LDS_PTR(uint64_t))&s_dummy[w * 64];
    s_dummy[t] = ~0ull; if (kw::lane() == 0) s_word[w] = ~0ull;
    kw::lds_order();
    kfl_write(word, r[3], dummy);
    kw::lds_order();
    o[3] = kfl_read(word); o[4] = *word; o[5] = s_dummy[t];
}
// in: val, address 0 .. 3, bits            out (seven words per address, preset by the caller): atomic_add(double), atomic_add / atomic_min / atomic_max (int32, the word's
// low half), atomic_add / atomic_or (64 bits), atomic_or32 (the word's low half)
KW_BODY void atomics(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(); const int val = (int)in[3 * g]; uint64_t* o = out + 7 * (in[3 * g + 1] & 3); const uint64_t bits = in[3 * g + 2];
    (void)kw::atomic_add(reinterpret_cast<double*>(o), (double)val);
    (void)kw::atomic_add(reinterpret_cast<int32_t*>(o + 1), val); (void)kw::atomic_min(reinterpret_cast<int32_t*>(o + 2), val); (void)kw::atomic_max(reinterpret_cast<int32_t*>(o + 3), val);
    (void)kw::atomic_add(reinterpret_cast<unsigned long long*>(o + 4), (unsigned long long)(uint32_t)val); (void)kw::atomic_or(reinterpret_cast<unsigned long long*>(o + 5), (unsigned long long)bits);
    (void)kw::atomic_or32(reinterpret_cast<uint32_t*>(o + 6), (uint32_t)(bits >> 17));
}
// in: a, b (nw / 2 records; the threads beyond do nothing)       out: bk_div_small(a, b), kfl_div(a, b) where b <= 8 (else 0)
KW_BODY void div_small(const uint64_t* in, uint64_t* out, int64_t nw) {
    const int g = gidx(); if (g >= nw / 2) return;
    const int a = (int)in[2 * g], b = (int)in[2 * g + 1];
    out[2 * g] = word_of(bk_div_small(a, b)); out[2 * g + 1] = word_of(b <= 8 ? kfl_div(a, b) : 0);
}
// in: LV (the table of the thread's own lane)             out: kfl_tab(lane, LV); kfl_quot(tab, g) for g = 0 .. 8 (0 beyond LV)
KW_BODY void kfl_table(const uint64_t* in, uint64_t* out, int64_t) {
    const int g = gidx(), LV = (int)in[g]; uint64_t* o = out + 10 * g;
    const uint32_t tab = kfl_tab(kw::lane(), LV);
    o[0] = tab; for (int q = 0; q <= 8; q++) o[1 + q] = word_of(q <= LV ? kfl_quot(tab, q) : 0);
}

// id, body, input words per thread, output words per thread (0: the buffers are laid out otherwise, see the body; kwc_run checks those sizes itself)
#define KWC_CASES(X) \
    X(0, scan_int, 1, 1) X(1, scan_f64, 1, 1) X(2, wave_max, 2, 5) X(3, key_scan, 10, 4) X(4, block_add3, 3, 12) X(5, block_add6, 6, 24) X(6, block_max, 16, 16) X(7, block_excl, 16, 20) \
    X(8, wg_scan, 2, 4) X(9, plan_setup, 0, 0) X(10, lane_ops, 3, 11) X(11, shfl, 2, 18) X(12, ballot_rank, 2, 2) X(13, scalar_bits, 2, 4) X(14, lds_ops, 4, 6) X(15, atomics, 3, 0) \
    X(16, div_small, 0, 0) X(17, kfl_table, 1, 10)

// the buffers a launch needs, in bytes, or false for a shape the case does not take: checked before anything is launched, so that no body indexes past a buffer
inline bool sizes_ok(int case_id, size_t in_bytes, size_t out_bytes, int grid, int block) {
    if (grid < 1 || grid > 4096 || block < 1 || block > 1024) return false;
    const size_t threads = (size_t)grid * block;
    switch (case_id) {
#define KWC_X(id, name, iw, ow) case id: if (iw && in_bytes < threads * iw * 8) return false; if (ow && out_bytes < threads * ow * 8) return false; break;
        KWC_CASES(KWC_X)
#undef KWC_X
        default: return false;
    }
    if (case_id == 9) {  // plan_setup: one workgroup; Q is not known before the input is read, so the caller passes buffers for M = (in_bytes / 4 - 3) / 4 nodes
        if (grid != 1 || in_bytes < 28) return false;
        const size_t M = (in_bytes / 4 - 3) / 4;
        return out_bytes >= (7 * M + 2) * 4 + M;
    }
    if (case_id == 15) return out_bytes >= 4 * 7 * 8;
    if (case_id == 16) return in_bytes % 16 == 0 && out_bytes >= in_bytes;
    if (case_id >= 4 && case_id <= 7) return block % 64 == 0;  // PlanScanLds: whole wavefronts, 16 at most
    return true;
}
// plan_setup reads Q from the buffer: the launcher compares it with the buffers' sizes before the launch
inline bool plan_setup_q_ok(const void* in, size_t in_bytes) {
    const int32_t* p = static_cast<const int32_t*>(in); const int32_t q = p[0];
    if (q < 0 || (size_t)q + 1 != (in_bytes / 4 - 3) / 4) return false;  // (4 M + 3 words, padded to whole 64-bit words)
    for (int i = 0; i <= q; i++) if (p[3 + 3 * (q + 1) + i] < 0 || p[3 + 3 * (q + 1) + i] > q) return false;  // h_nodes: the body indexes with them
    return true;
}
}  // namespace kwc
