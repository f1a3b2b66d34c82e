// fill_replay.cpp — TEST INFRASTRUCTURE: replays ONE fill launch given as a file (the format of host_sim.cpp's KAI_HOSTSIM_FILL_DUMP, <prefix>.in) through the emulated k_fill_levels
// and k_fill_counts (kai_simt.hpp's host emulator: KW_EMU_ORDER / KW_EMU_SEED are read once per process) and through the scalar C++ fill of native_bucket_fill.hpp, compares every
// output and every counter of the three, and writes k_fill_levels' outputs as <prefix>.out.  What tools/micro/fill_bench.hip does on the MI355X, on the CPU — for launches a test
// writes itself: inputs the kernels must handle that no plan of the engine produces (tests/test_fill_levels_runs.py).
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread -o fill_replay tests/host_sim/fill_replay.cpp ; fill_replay <prefix>      exit status 0: all equal
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../kai-scheduler_amd/csrc/kai_host_prep.hpp"
#include "../../kai-scheduler_amd/csrc/kai_batch_kernels.hpp"
#include "native_bucket_fill.hpp"

using namespace kai;
using kai_native::NativeFillOut; using kai_native::native_fill_buckets;

template <class T> static void rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: fill_replay <prefix>\n"); return 2; }
    const std::string pre = argv[1];
    FILE* f = std::fopen((pre + ".in").c_str(), "rb"); if (!f) { std::perror("in"); return 2; }
    int32_t hdr[16]; RoundParams rp; BucketParams bp;
    if (std::fread(hdr, 4, 16, f) != 16 || std::fread(&rp, sizeof rp, 1, f) != 1 || std::fread(&bp, sizeof bp, 1, f) != 1 || hdr[0] != 0x4b464c31) { std::fprintf(stderr, "bad header\n"); return 2; }
    const int C = hdr[1], Q = hdr[2], P = hdr[3], V = hdr[4], LV = hdr[5], NW = hdr[6];
    if (LV != bp.levels || NW != bp.nw || LV > KFL_LMAX || bp.n_ok != 0) { std::fprintf(stderr, "not a launch of k_fill_levels\n"); return 2; }
    std::vector<double> qd; rd(f, qd, 64);
    std::vector<uint8_t> g_flag; std::vector<int32_t> g_first, g_nt, g_ucls, t_cls; std::vector<uint64_t> words;
    rd(f, g_flag, V); rd(f, g_first, V); rd(f, g_nt, V); rd(f, g_ucls, V); rd(f, t_cls, P); rd(f, words, (size_t)LV * NW); std::fclose(f);

    std::vector<ClassRec> cls(64); for (int k = 0; k < 64; k++) { std::memset((void*)&cls[k], 0, sizeof(ClassRec)); cls[k].req[KAI_RES_GPU] = qd[k]; }
    std::vector<int32_t> q_valid(Q + 1, 0); q_valid[Q] = V;
    const size_t dyn = ((size_t)LV * NW + (size_t)LV * bp.nw1 + KBK_GMAX) * 8 + 16;  // the sets and their first summaries (kai_batch_driver.hpp batch_bucket_params; a plain cluster has no class bitmaps)

    struct Out { std::vector<uint64_t> words; std::vector<uint8_t> g_out; std::vector<int32_t> g_opoff, g_stmt, t_node; FillStatus fs; };
    auto run = [&](int kern, Out& o, NativeFillOut* nat) {
        o.words.assign((size_t)KBK_GMAX * NW, 0); std::copy(words.begin(), words.end(), o.words.begin());
        o.g_out.assign(V + 64, 0); o.g_opoff.assign(V + 64, 0); o.g_stmt.assign(V + 64, 0); o.t_node.assign(P + 64, -1); std::memset((void*)&o.fs, 0, sizeof o.fs);
        uint64_t dead = 0;
        KaiCtx c; std::memset((void*)&c, 0, sizeof c);
        c.C = C; c.Q = Q; c.P = P; c.NB = NW; c.cls = cls.data();
        BatchCtx& b = c.bt;
        b.q_valid = q_valid.data(); b.g_flag = g_flag.data(); b.g_first = g_first.data(); b.g_nt = g_nt.data(); b.g_ucls = g_ucls.data(); b.t_cls = t_cls.data();
        b.bk_words = o.words.data(); b.g_out = o.g_out.data(); b.g_opoff = o.g_opoff.data(); b.g_stmt = o.g_stmt.data(); b.t_node = o.t_node.data(); b.fs = &o.fs; b.dead_mask = &dead;
        if (nat) { native_fill_buckets(c, rp, bp, *nat); return; }
        if (kern == 0) kw::launch(1, 64 * (LV + 2), dyn, [&] { kb_fill_levels(c, rp, bp); });
        else kw::launch(1, 256, dyn, [&] { kb_fill_counts(c, rp, bp); });
    };
    Out lev, cnt, scratch; NativeFillOut nat;
    run(0, scratch, &nat); run(0, lev, nullptr); run(1, cnt, nullptr);

    long long bad = 0;
    auto same_fs = [&](const FillStatus& a, const FillStatus& x, const char* who) {
        if (a.n_done != x.n_done || a.mismatch != x.mismatch || a.decisions != x.decisions || a.attempted != x.attempted || a.committed != x.committed || a.rollbacks != x.rollbacks || a.ops != x.ops ||
            a.dead_mask != x.dead_mask || a.all_dead != x.all_dead) {
            bad++; std::fprintf(stderr, "%s: counters differ: n_done %d/%d mismatch %d/%d decisions %lld/%lld attempted %lld/%lld committed %lld/%lld rollbacks %lld/%lld ops %lld/%lld\n", who, a.n_done, x.n_done, a.mismatch,
                                x.mismatch, (long long)a.decisions, (long long)x.decisions, (long long)a.attempted, (long long)x.attempted, (long long)a.committed, (long long)x.committed, (long long)a.rollbacks, (long long)x.rollbacks, (long long)a.ops, (long long)x.ops);
        }
    };
    same_fs(lev.fs, nat.fs, "k_fill_levels against the scalar fill"); same_fs(cnt.fs, nat.fs, "k_fill_counts against the scalar fill");
    if (lev.fs.rescans2 != cnt.fs.rescans2) { bad++; std::fprintf(stderr, "commands differ: %lld / %lld\n", (long long)lev.fs.rescans2, (long long)cnt.fs.rescans2); }
    for (const Out* o : {&lev, &cnt}) {
        for (int gi = rp.start; gi < nat.fs.n_done && gi < V; gi++) {
            const int x = gi - rp.start;
            if (o->g_out[gi] != nat.g_out[x]) { bad++; continue; }
            if (nat.g_out[x] != BF_OK || g_flag[gi] == BF_GATE) continue;
            if (o->g_opoff[gi] != nat.g_opoff[x] || o->g_stmt[gi] != nat.g_stmt[x]) bad++;
            for (int t = 0; t < g_nt[gi]; t++) if (o->t_node[g_first[gi] + t] != nat.t_node[(size_t)g_first[gi] + t]) bad++;
        }
        for (size_t i = 0; i < (size_t)LV * NW; i++) if (o->words[i] != nat.words[i]) bad++;
    }
    f = std::fopen((pre + ".out").c_str(), "wb"); if (!f) { std::perror("out"); return 2; }
    std::fwrite(&lev.fs, sizeof lev.fs, 1, f); std::fwrite(lev.g_out.data(), 1, V, f); std::fwrite(lev.g_opoff.data(), 4, V, f); std::fwrite(lev.g_stmt.data(), 4, V, f);
    std::fwrite(lev.t_node.data(), 4, P, f); std::fwrite(lev.words.data(), 8, (size_t)LV * NW, f); std::fclose(f);
    std::printf("executed %d mismatch %d decisions %lld committed %lld rollbacks %lld commands %lld: %lld differences\n", lev.fs.n_done, lev.fs.mismatch, (long long)lev.fs.decisions, (long long)lev.fs.committed,
                (long long)lev.fs.rollbacks, (long long)lev.fs.rescans2, bad);
    return bad ? 1 : 0;
}
