// kw_conformance_sim.cpp — TEST INFRASTRUCTURE: the bodies of kw_conformance.hpp compiled with plain g++ and run on the lock-step emulator of kai_simt.hpp, behind the same
// kwc_run as the device library (kw_conformance.hip).  tests/test_kw_conformance.py builds it and compares it with the case table of tests/kw_conformance_cases.py.
// -DKWC_MAIN adds a main() that runs every case once on fixed inputs against values computed below in plain C++: the stand-alone program the sanitizers are run on.
#define KAI_SHARED_GPUS 1
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../../kai-scheduler_amd/csrc/kai_host_prep.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_kernels.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_driver.hpp"
#include "../../kai-scheduler_amd/csrc/kai_victim_shard.hpp"
#include "../../kai-scheduler_amd/csrc/kai_stale_gangs.hpp"
#include "kw_conformance.hpp"

// the device library's contract: 0, or 1 (hipErrorInvalidValue) without a launch for buffers too small for the shape.  The emulator works on the caller's buffers.
extern "C" int kwc_run(int case_id, const void* in, size_t in_bytes, void* out, size_t out_bytes, int grid, int block) {
    if (!in || !out || !kwc::sizes_ok(case_id, in_bytes, out_bytes, grid, block)) return 1;
    if (case_id == 9 && !kwc::plan_setup_q_ok(in, in_bytes)) return 1;
    const uint64_t* i64 = static_cast<const uint64_t*>(in); uint64_t* o64 = static_cast<uint64_t*>(out); const int64_t nw = (int64_t)(in_bytes / 8);
    switch (case_id) {
#define KWC_X(id, name, iw, ow) case id: kw::launch(grid, block, 0, [&] { kwc::name(i64, o64, nw); }); break;
        KWC_CASES(KWC_X)
#undef KWC_X
    }
    return 0;
}

#ifdef KWC_MAIN
// Every body once, two workgroups of 128 lanes (100 where the product runs partial workgroups), inputs from a fixed generator, against plain serial C++.
namespace {
uint64_t g_s = 0x243f6a8885a308d3ull;
uint64_t rnd() { g_s = g_s * 6364136223846793005ull + 1442695040888963407ull; uint64_t x = g_s; x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 29; return x; }
int g_bad = 0;
void expect(bool ok, const char* what, long at) { if (!ok && g_bad++ < 20) std::fprintf(stderr, "kw_conformance_sim: %s differs at %ld\n", what, at); }
using Words = std::vector<uint64_t>;
enum { C_SCAN_INT, C_SCAN_F64, C_WAVE_MAX, C_KEY_SCAN, C_BLOCK_ADD3, C_BLOCK_ADD6, C_BLOCK_MAX, C_BLOCK_EXCL, C_WG_SCAN, C_PLAN_SETUP, C_LANE_OPS, C_SHFL, C_BALLOT_RANK, C_SCALAR_BITS, C_LDS_OPS, C_ATOMICS, C_DIV, C_KFL_TABLE };
Words run(int id, const Words& in, size_t out_words, int grid, int block, uint64_t preset = 0xA5A5A5A5A5A5A5A5ull) {
    Words out(out_words, preset);
    const int rc = kwc_run(id, in.data(), in.size() * 8, out.data(), out.size() * 8, grid, block);
    if (rc) { std::fprintf(stderr, "kw_conformance_sim: kwc_run(%d) returned %d\n", id, rc); g_bad++; }
    return out;
}
struct Key { uint64_t w[4]; bool operator<(const Key& o) const { for (int i = 0; i < 4; i++) if (w[i] != o.w[i]) return w[i] < o.w[i]; return false; } };
Key key_of(const uint64_t* p) { Key k; for (int i = 0; i < 4; i++) k.w[i] = p[i]; return k; }
bool key_eq(const uint64_t* p, const Key& k) { return p[0] == k.w[0] && p[1] == k.w[1] && p[2] == k.w[2] && p[3] == k.w[3]; }
double f64(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
uint64_t bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
}  // namespace

int main() {
    const int G = 2, B = 128, T = G * B;
    {   // the two wave scans
        Words in(T), inf(T);
        for (int i = 0; i < T; i++) { in[i] = (uint64_t)(int64_t)((int)(rnd() % 2000001) - 1000000); inf[i] = bits((double)(rnd() >> 24)); }
        const Words o = run(C_SCAN_INT, in, T, G, B), of = run(C_SCAN_F64, inf, T, G, B);
        int64_t s = 0; double sf = 0;
        for (int i = 0; i < T; i++) { if (i % 64 == 0) { s = 0; sf = 0; } s += (int64_t)in[i]; sf += f64(inf[i]); expect((int64_t)o[i] == s, "wave_scan_add<int>", i); expect(of[i] == bits(sf), "wave_scan_add<double>", i); }
        const Words o100 = run(C_SCAN_INT, Words(in.begin(), in.begin() + 100), 100, 1, 100);
        s = 0; for (int i = 0; i < 100; i++) { if (i % 64 == 0) s = 0; s += (int64_t)in[i]; expect((int64_t)o100[i] == s, "wave_scan_add<int> at 100 lanes", i); }
    }
    {   // maximum and arg-max: a few values, so that lanes tie
        Words in(2 * T);
        for (int i = 0; i < T; i++) { in[2 * i] = (rnd() % 5) << 61 | (rnd() % 3); in[2 * i + 1] = (uint64_t)(int64_t)(i * 7 - 300); }
        const Words o = run(C_WAVE_MAX, in, 5 * T, G, B);
        for (int w = 0; w < T / 64; w++) {
            uint64_t m = 0; int first = 0;
            for (int l = 0; l < 64; l++) if (in[2 * (64 * w + l)] > m) { m = in[2 * (64 * w + l)]; first = l; }
            for (int l = 0; l < 64; l++) { const uint64_t* p = &o[5 * (64 * w + l)]; expect(p[0] == m && p[1] == m && p[3] == m && p[2] == in[2 * (64 * w + first) + 1] && p[4] == p[2], "wave_max_u64 / wave_argmax_first", 64 * w + l); }
        }
    }
    {   // keys: per wavefront, then over the workgroup (inclusive and exclusive), two calls in a row
        Words in(10 * T), inb(16 * T);
        for (int i = 0; i < T; i++) {
            uint64_t* r = &in[10 * i]; r[0] = rnd() % 3; r[1] = rnd(); r[2] = rnd(); r[3] = rnd(); r[4] = rnd() % 3 == 0; r[5] = i >= B; r[6] = 1; r[7] = r[8] = r[9] = 0;
            uint64_t* q = &inb[16 * i]; for (int k = 0; k < 4; k++) { q[k] = k ? rnd() : rnd() % 3; q[5 + k] = k ? rnd() : rnd() % 3; }
            q[4] = rnd() % 4 == 0 && (i % B) >= 70; q[9] = rnd() % 2; q[10] = i >= B; q[11] = 1; q[12] = q[13] = q[14] = 5; q[15] = 1;  // (the first wavefront of a holds no key; have2: a carry, or a key of a)
        }
        for (int g = 0; g < G; g++) { bool any = inb[16 * g * B + 10] != 0; for (int t = 0; t < B; t++) any = any || inb[16 * (g * B + t) + 4]; for (int t = 0; t < B; t++) inb[16 * (g * B + t) + 15] = any; }
        const Words o = run(C_KEY_SCAN, in, 4 * T, G, B);
        for (int w = 0; w < T / 64; w++) {
            bool have = in[10 * 64 * w + 5] != 0; Key cur = key_of(&in[10 * 64 * w + 6]);
            for (int l = 0; l < 64; l++) { const uint64_t* r = &in[10 * (64 * w + l)]; if (r[4] && (!have || cur < key_of(r))) { cur = key_of(r); have = true; } if (have) expect(key_eq(&o[4 * (64 * w + l)], cur), "kb_wave_scan_max", 64 * w + l); }
        }
        const Words om = run(C_BLOCK_MAX, inb, 16 * T, G, B), ox = run(C_BLOCK_EXCL, inb, 20 * T, G, B);
        for (int g = 0; g < G; g++) {
            bool have = inb[16 * g * B + 10] != 0; Key cur = key_of(&inb[16 * g * B + 11]);
            std::vector<Key> inc(2 * B), exc(2 * B); std::vector<char> hi(2 * B), he(2 * B); Key last[2]; bool hl[2];
            for (int call = 0; call < 2; call++) {
                for (int t = 0; t < B; t++) {
                    const uint64_t* r = &inb[16 * (g * B + t) + 5 * call];
                    exc[call * B + t] = cur; he[call * B + t] = have;
                    if (r[4] && (!have || cur < key_of(r))) { cur = key_of(r); have = true; }
                    inc[call * B + t] = cur; hi[call * B + t] = have;
                }
                last[call] = cur; hl[call] = have;
            }
            for (int t = 0; t < B; t++) for (int call = 0; call < 2; call++) {
                const uint64_t* m = &om[16 * (g * B + t) + 8 * call]; const uint64_t* x = &ox[20 * (g * B + t) + 10 * call]; const int i = call * B + t;
                if (hi[i]) expect(key_eq(m, inc[i]), "kb_block_scan_max", g * B + t);
                if (hl[call]) expect(key_eq(m + 4, last[call]) && key_eq(x + 5, last[call]), "kb_block_scan_max / kb_block_excl_max: last", g * B + t);
                expect(x[4] == (uint64_t)he[i] && x[9] == (uint64_t)hl[call], "kb_block_excl_max: have_pre / have_last", g * B + t);
                if (he[i]) expect(key_eq(x, exc[i]), "kb_block_excl_max", g * B + t);
            }
        }
    }
    for (int nv : {3, 6}) {   // sums over the workgroup, the second call carrying the first one's totals
        Words in((size_t)nv * T);
        for (auto& x : in) x = bits((double)(rnd() >> 26) / 1024.0);
        const Words o = run(nv == 3 ? C_BLOCK_ADD3 : C_BLOCK_ADD6, in, (size_t)4 * nv * T, G, B);
        for (int g = 0; g < G; g++) for (int k = 0; k < nv; k++) {
            double tot = 0; for (int t = 0; t < B; t++) tot += f64(in[(size_t)nv * (g * B + t) + k]);
            double s1 = 0, s2 = tot; const double d0 = f64(in[(size_t)nv * g * B + k]);  // the second call: twice the values, thread 0 its own plus the first call's total
            for (int t = 0; t < B; t++) {
                const double d = f64(in[(size_t)nv * (g * B + t) + k]); s1 += d; s2 += t ? d + d : d; const uint64_t* p = &o[(size_t)4 * nv * (g * B + t)];
                expect(p[k] == bits(s1) && p[nv + k] == bits(tot) && p[2 * nv + k] == bits(s2) && p[3 * nv + k] == bits(tot + tot + tot - d0), "kb_block_scan_add", g * B + t);
            }
        }
    }
    {   // sg_wg_scan at 100 lanes, the packed word; kb_plan_setup on 300 nodes
        Words in(2 * 100);
        for (int i = 0; i < 100; i++) { in[2 * i] = rnd() % 3 == 0 ? (1 | 1 << 16) : rnd() % 2; in[2 * i + 1] = rnd() % 1000; }
        const Words o = run(C_WG_SCAN, in, 4 * 100, 1, 100);
        int64_t t1 = 0, t2 = 0, s1 = 0, s2 = 0; for (int i = 0; i < 100; i++) { t1 += (int64_t)in[2 * i]; t2 += (int64_t)in[2 * i + 1]; }
        for (int i = 0; i < 100; i++) { s1 += (int64_t)in[2 * i]; s2 += (int64_t)in[2 * i + 1]; expect((int64_t)o[4 * i] == s1 && (int64_t)o[4 * i + 1] == t1 && (int64_t)o[4 * i + 2] == s2 && (int64_t)o[4 * i + 3] == t2, "sg_wg_scan", i); }
        const int M = 300, Q = M - 1, H = 8;
        std::vector<int32_t> a(4 * M + 4, 0); a[0] = Q; a[1] = H;
        int32_t* off = &a[2]; int32_t* cur = &a[3 + M]; int32_t* end = &a[3 + 2 * M]; int32_t* hn = &a[3 + 3 * M];
        for (int q = 0; q < M; q++) { off[q + 1] = off[q] + (rnd() % 5 == 0 ? 1 + (int)(rnd() % 4) : 0); cur[q] = (int)(rnd() % 40); end[q] = cur[q] + (int)(rnd() % 23) - 2; hn[q] = (int)(((int64_t)q * 7 + 11) % M); }
        Words in64((a.size() + 1) / 2); std::memcpy(in64.data(), a.data(), a.size() * 4);
        const size_t ob = (size_t)(7 * M + 2) * 4 + M;
        const Words o64 = run(C_PLAN_SETUP, in64, (ob + 7) / 8, 1, B);
        const int32_t* o32 = reinterpret_cast<const int32_t*>(o64.data());
        int se = 0, sk = 0;
        for (int i = 0; i < M; i++) {
            const int x = hn[i], nch = off[x + 1] - off[x]; int cnt = 0;
            if (x < Q && nch == 0) { cnt = std::min(end[x] - cur[x], H); if (cnt < 0) cnt = 0; }
            expect(o32[x] == se && o32[M + x] == sk && o32[2 * M + x] == cnt && o32[3 * M + x] == 0x7fffffff && o32[4 * M + x] == 0 && o32[5 * M + x] == 0 && o32[6 * M + x] == 0, "kb_plan_setup", x);
            se += cnt + nch; sk += cnt + 1;
        }
        expect(o32[7 * M] == se && o32[7 * M + 1] == sk, "kb_plan_setup: plan_tot", 0);
    }
    {   // lanes: bcast / uni / writelane / opaque, shfl / shfl_up, ballot / rank_below
        Words in(3 * T), ins(2 * T), inb(2 * T);
        std::vector<uint64_t> u(T / 64), m(T / 64); std::vector<int> src(T / 64);
        for (int w = 0; w < T / 64; w++) { u[w] = rnd(); m[w] = rnd(); src[w] = (int)(rnd() % 64); }
        for (int i = 0; i < T; i++) { in[3 * i] = rnd(); in[3 * i + 1] = u[i / 64]; in[3 * i + 2] = (uint64_t)src[i / 64]; ins[2 * i] = rnd(); ins[2 * i + 1] = rnd() % 64; inb[2 * i] = rnd() % 2; inb[2 * i + 1] = m[i / 64]; }
        const Words o = run(C_LANE_OPS, in, 11 * T, G, B), os = run(C_SHFL, ins, 18 * T, G, B), ob = run(C_BALLOT_RANK, inb, 2 * T, G, B);
        const int ds[7] = {1, 2, 4, 8, 16, 32, 63};
        for (int i = 0; i < T; i++) {
            const int w = i / 64, l = i % 64; const uint64_t v = in[3 * i], vs = in[3 * (64 * w + src[w])], uu = u[w]; const uint64_t* p = &o[11 * i];
            expect(p[0] == (uint64_t)(int64_t)(int)vs && p[1] == vs >> 32 && p[2] == vs && p[3] == vs && p[4] == (uint64_t)(int64_t)(int)uu && p[5] == uu >> 32 && p[6] == uu, "bcast / uni", i);
            expect(p[7] == (uint64_t)(int64_t)(int)(l == src[w] ? uu : v) && p[8] == (l == src[w] ? uu : v) && p[9] == uu && p[10] == (uint32_t)uu, "writelane / opaque", i);
            const uint64_t f = ins[2 * (64 * w + (int)ins[2 * i + 1])]; const uint64_t* q = &os[18 * i];
            expect(q[0] == (uint64_t)(int64_t)(int)f && q[1] == f && q[2] == f && q[3] == f, "shfl", i);
            for (int k = 0; k < 7; k++) { const uint64_t e = ins[2 * (l >= ds[k] ? i - ds[k] : i)]; expect(q[4 + k] == (uint64_t)(int64_t)(int)e && q[11 + k] == e, "shfl_up", i); }
            uint64_t bal = 0; for (int j = 0; j < 64; j++) if (inb[2 * (64 * w + j)]) bal |= 1ull << j;
            expect(ob[2 * i] == bal && ob[2 * i + 1] == (uint64_t)__builtin_popcountll(m[w] & ((1ull << l) - 1)), "ballot / rank_below", i);
        }
    }
    {   // uniform bit operations, LDS words, atomics
        Words in(2 * T), inl(4 * T), ina(3 * T);
        for (int i = 0; i < T; i++) { if (i % 64 == 0) { in[2 * i] = rnd() % 4 ? rnd() : 0; in[2 * i + 1] = rnd() % 128; } else { in[2 * i] = in[2 * (i - 1)]; in[2 * i + 1] = in[2 * (i - 1) + 1]; } }
        for (auto& x : inl) x = rnd();
        for (int i = 0; i < T; i++) { ina[3 * i] = (uint64_t)(int64_t)((int)(rnd() % 60001) - 30000); ina[3 * i + 1] = rnd() % 4; ina[3 * i + 2] = rnd() & rnd(); }
        const Words o = run(C_SCALAR_BITS, in, 4 * T, G, B), ol = run(C_LDS_OPS, inl, 6 * T, G, B);
        for (int i = 0; i < T; i++) {
            const uint64_t v = in[2 * i]; const int b = (int)in[2 * i + 1]; const uint32_t v32 = (uint32_t)v;
            expect(o[4 * i] == (v32 ? 1u : 0u) && o[4 * i + 1] == (v32 & ~(1u << (b & 31))) && o[4 * i + 2] == (v32 | (1u << (b & 31))) && o[4 * i + 3] == (v & ~(1ull << (b & 63))), "nonzero01 / bit_clear / bit_set", i);
            const uint64_t* r = &inl[4 * i]; const uint64_t x = (r[0] ^ r[1]) | r[2], first = inl[4 * (i & ~63) + 3];
            expect(ol[6 * i] == r[0] && ol[6 * i + 1] == x && ol[6 * i + 2] == (x ^ r[0]) && ol[6 * i + 3] == first && ol[6 * i + 4] == first && ol[6 * i + 5] == (i % 64 ? r[3] : ~0ull), "lds_xor / lds_or / kfl_write / kfl_read", i);
        }
        Words out(28, 0); for (int k = 0; k < 4; k++) { out[7 * k + 2] = 0x7fffffff; out[7 * k + 3] = 0x80000000u; }
        if (kwc_run(C_ATOMICS, ina.data(), ina.size() * 8, out.data(), out.size() * 8, G, B)) g_bad++;
        for (int k = 0; k < 4; k++) {
            int64_t s = 0; int mn = 0x7fffffff, mx = -0x7fffffff - 1; uint64_t su = 0, orr = 0;
            for (int i = 0; i < T; i++) if ((int)ina[3 * i + 1] == k) { const int v = (int)ina[3 * i]; s += v; mn = std::min(mn, v); mx = std::max(mx, v); su += (uint32_t)v; orr |= ina[3 * i + 2]; }
            const uint64_t* p = &out[7 * k];
            expect(p[0] == bits((double)s) && p[1] == (uint32_t)s && p[2] == (uint32_t)mn && p[3] == (uint32_t)mx && p[4] == su && p[5] == orr && p[6] == (uint32_t)(orr >> 17), "atomics", k);
        }
    }
    {   // the small divisions, every pair; the quotient tables
        Words in; for (int a = 0; a <= 1024; a++) for (int b = 1; b <= 64; b++) { in.push_back((uint64_t)a); in.push_back((uint64_t)b); }
        const int n = (int)in.size() / 2;
        const Words o = run(C_DIV, in, in.size(), (n + 1023) / 1024, 1024);
        for (int i = 0; i < n; i++) { const int a = (int)in[2 * i], b = (int)in[2 * i + 1]; expect((int)o[2 * i] == a / b && (int)o[2 * i + 1] == (b <= 8 ? a / b : 0), "bk_div_small / kfl_div", i); }
        Words lv(512); for (int i = 0; i < 512; i++) lv[i] = (uint64_t)(i / 64 + 1);
        const Words ot = run(C_KFL_TABLE, lv, 5120, 8, 64);
        for (int i = 0; i < 512; i++) for (int g = 0; g <= 8; g++) expect((int)ot[10 * i + 1 + g] == (g <= i / 64 + 1 ? g / (i % 64 + 1) : 0), "kfl_tab / kfl_quot", i);
    }
    for (char* st : kw::emu().stacks) std::free(st);  // the emulator keeps its fibers' stacks for the life of the process: handed back so that a leak check ends clean
    kw::emu().stacks.clear();
    if (g_bad) { std::fprintf(stderr, "kw_conformance_sim: %d differences\n", g_bad); return 1; }
    std::printf("kw_conformance_sim: ok\n");
    return 0;
}
#endif
