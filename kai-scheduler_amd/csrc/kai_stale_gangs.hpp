// kai_stale_gangs.hpp — kai_stale_gang_eviction: the default cycle's fifth action (actions/stalegangeviction/stalegangeviction.go:29-90) decided on the device against
// the session's current state and applied by kai_ops_apply's own kernels.
//
//   k_sg_succeeded  a thread per pod: a Succeeded pod sets its job's flag in the handle's scratch (every writer stores the same value).
//   k_sg_jobs       a thread per job: PodGroupInfo.IsStale (api/podgroup_info/job_info.go:417-432) from the flag and the job's pod-sets, the new staleness timestamp,
//                   whether the grace period ran out (StalenessInfo.Stale), the two result counters (one atomic per wavefront).  Clears the flag it read: the scratch is
//                   zero between calls.
//   k_sg_first      a thread per pod: the lowest evicted pod of every expired job, through an atomic minimum.
//   k_sg_totals     a thread per pod: two flags — "this pod is evicted" (its job expired, its status is active-allocated) and "it is the first such pod of its job" —
//                   summed per workgroup.
//   k_sg_scan       ONE workgroup: the exclusive scan of the workgroups' totals, in place, in tiles of the workgroup's size with a carry; the call's two counts.
//   k_sg_emit       a thread per pod: the flags again, scanned inside the workgroup; the kai_op list in ascending pod index behind an OaHead, where OaLayout puts it:
//                   the first scan is the operation's position and seq, the second its stmt (one number per job with an eviction, in array order).
// The apply is oa_drive (kai_ops_apply.hpp) on that device-resident list: nothing of the accounting is written here.
//
// No kernel waits on another workgroup; every loop is bounded by a job's pod-sets, by the workgroups of the pod grid or by the wavefronts of a workgroup.
// The bodies are written against kai_simt.hpp: tests/host_sim/stale_gangs_sim.cpp runs them with emulated lanes.
#pragma once
#include "kai_ops_apply.hpp"

namespace kai {

constexpr int KAI_SG_WG = 256;  // lanes of a workgroup of every kernel here (the emulator also runs them with 100 and 1)
constexpr int32_t KAI_SG_NO_POD = 0x7fffffff;

// the call's counts: sent zeroed in front of the timestamps, read back before the apply
struct SgHead { int32_t stale_jobs, expired_jobs, n_ops, n_stmts, pad[12]; };
static_assert(sizeof(SgHead) == 64, "SgHead is one 64-byte record in front of the timestamps");

struct SgArgs {
    int64_t now_ns, grace_ns;
    int32_t n_wgs, pad;           // workgroups of the pod grid (k_sg_totals / k_sg_emit)
    KAI_GP(SgHead) head;
    KAI_GP(int64_t) since;        // [J] in: the caller's timestamps; out: what the reference leaves in StalenessInfo.TimeStamp (0 = nil)
    KAI_GP(uint8_t) expired;      // [J] the grace period ran out this call: StalenessInfo.Stale
    KAI_GP(int32_t) succ;         // [J] the job has a Succeeded pod; zero between calls
    KAI_GP(int32_t) first;        // [J] lowest evicted pod of the job (KAI_SG_NO_POD: none)
    KAI_GP(int32_t) wg_e, wg_f;   // [n_wgs] per workgroup of the pod grid: evicted pods / first evicted pods, then their exclusive scans
    KAI_GP(OaHead) oa_head;       // what k_sg_emit writes for oa_drive
    KAI_GP(kai_op) ops;           // [n_ops] node = name rank
};

// Where the pieces lie in the handle's scratch: offsets depend on the capacities only, so that the zeroed flags stay where they are while the scratch is large enough.
struct SgLayout {
    size_t head, since, expired, succ, first, wg_e, wg_f, end;
    SgLayout(size_t job_cap, size_t wg_cap) {
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        size_t o = 0;
        head = o; o += sizeof(SgHead);
        since = o; o = al(o + job_cap * 8);  // [head | since] is what every call sends
        expired = o; o = al(o + job_cap);
        succ = o; o = al(o + job_cap * 4);
        first = o; o = al(o + job_cap * 4);
        wg_e = o; o = al(o + wg_cap * 4);
        wg_f = o; o = al(o + wg_cap * 4);
        end = o;
    }
};

KW_BODY void sg_succeeded_body(const KaiCtx& c, const SgArgs& a) {
    const int64_t p = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (p < c.P && c.p_status[p] == KAI_POD_SUCCEEDED) a.succ[c.p_job[p]] = 1;
}

KW_BODY void sg_jobs_body(const KaiCtx& c, const SgArgs& a) {
    const int64_t j = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    bool stale = false, expired = false;
    if (j < c.J) {
        const bool succeeded = a.succ[j] != 0;
        a.succ[j] = 0;
        int active = 0; bool unsatisfied = false;
        for (int k = 0; k < c.j_n_ps[j]; k++) {
            const int s = c.j_first_ps[j] + k, used = c.s_active_used[s];
            active += used;
            if (used < c.s_min[s]) unsatisfied = true;  // PodSet.IsGangSatisfied fails
        }
        stale = !succeeded && active > 0 && unsatisfied;
        const int64_t since = stale ? (a.since[j] != 0 ? a.since[j] : a.now_ns) : 0;
        expired = stale && a.grace_ns >= 0 && a.now_ns - since >= a.grace_ns;
        a.since[j] = since; a.expired[j] = expired ? 1 : 0; a.first[j] = KAI_SG_NO_POD;
    }
    const uint64_t ms = kw::ballot(stale), me = kw::ballot(expired);
    if (kw::lane() == 0) {  // (no lane left before the ballots: lane 0 is there)
        if (ms) kw::atomic_add((int32_t*)&a.head->stale_jobs, __builtin_popcountll(ms));
        if (me) kw::atomic_add((int32_t*)&a.head->expired_jobs, __builtin_popcountll(me));
    }
}

// this pod is evicted: its job's grace period ran out and it holds an active-allocated status (pod_status.go:66-67)
KW_BODY bool sg_evicted(const KaiCtx& c, const SgArgs& a, int64_t p) { return p < c.P && a.expired[c.p_job[p]] && st_active_allocated(c.p_status[p]); }

KW_BODY void sg_first_body(const KaiCtx& c, const SgArgs& a) {
    const int64_t p = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    if (sg_evicted(c, a, p)) kw::atomic_min((int32_t*)&a.first[c.p_job[p]], (int)p);
}

// Inclusive sums of v over the workgroup's lanes; total: the workgroup's sum.  s_w: one LDS word per wavefront.  Every lane of the workgroup calls it.
KW_BODY int sg_wg_scan(int v, int32_t* s_w, int& total) {
    const int tid = kw::tid(), w = tid >> 6, nw = (kw::bdim() + 63) >> 6;
    const int incl = kw::wave_scan_add(v);
    if (kw::lane() == 63 || tid == kw::bdim() - 1) s_w[w] = incl;
    kw::sync();
    int base = 0; total = 0;
    for (int k = 0; k < nw; k++) { const int t = s_w[k]; if (k < w) base += t; total += t; }
    kw::sync();  // (the words are written again by the next call)
    return incl + base;
}

// the pod's two flags in one word: the workgroup has at most 4096 lanes, so 16 bits hold either count
KW_BODY int sg_flags(const KaiCtx& c, const SgArgs& a, int64_t p) {
    if (!sg_evicted(c, a, p)) return 0;
    return 1 | (a.first[c.p_job[p]] == (int)p ? 1 << 16 : 0);
}

KW_BODY void sg_totals_body(const KaiCtx& c, const SgArgs& a) {
    KW_SHARED int32_t s_w[64];
    const int64_t p = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    int total = 0;
    (void)sg_wg_scan(sg_flags(c, a, p), s_w, total);
    if (kw::tid() == 0) { a.wg_e[kw::bid()] = total & 0xffff; a.wg_f[kw::bid()] = total >> 16; }
}

KW_BODY void sg_scan_body(const SgArgs& a) {
    KW_SHARED int32_t s_w[64];
    const int tid = kw::tid(), T = kw::bdim();
    int carry_e = 0, carry_f = 0;
    for (int base = 0; base < a.n_wgs; base += T) {  // (the same trip count in every lane)
        const int i = base + tid, e = i < a.n_wgs ? a.wg_e[i] : 0, f = i < a.n_wgs ? a.wg_f[i] : 0;
        int tot_e = 0, tot_f = 0;
        const int ie = sg_wg_scan(e, s_w, tot_e), jf = sg_wg_scan(f, s_w, tot_f);
        if (i < a.n_wgs) { a.wg_e[i] = carry_e + ie - e; a.wg_f[i] = carry_f + jf - f; }
        carry_e += tot_e; carry_f += tot_f;
    }
    if (tid == 0) { a.head->n_ops = carry_e; a.head->n_stmts = carry_f; }
}

KW_BODY void sg_emit_body(const KaiCtx& c, const SgArgs& a) {
    KW_SHARED int32_t s_w[64];
    const int64_t p = (int64_t)kw::bid() * kw::bdim() + kw::tid();
    const int v = sg_flags(c, a, p);
    int total = 0;
    const int incl = sg_wg_scan(v, s_w, total);
    if (v) {
        const int pos = a.wg_e[kw::bid()] + (incl & 0xffff) - 1, stmt = a.wg_f[kw::bid()] + (incl >> 16) - 1;
        a.ops[pos].seq = pos; a.ops[pos].kind = KAI_OP_EVICT; a.ops[pos].pod = (int32_t)p; a.ops[pos].node = c.p_node[p]; a.ops[pos].job = c.p_job[p];
        a.ops[pos].stmt = stmt; a.ops[pos].pad = 0;
    }
    if (p == 0) {
        a.oa_head->bad = KAI_OA_NONE; a.oa_head->dup = 0; a.oa_head->not_wide = 0; a.oa_head->applied = 0; a.oa_head->fault = 0; a.oa_head->fault_line = 0;
    }
}

// The call's control flow from its first launch on, written once against a Launcher that is oa_drive's Launcher (check, wide, engine, read_head) and also has
//   void succeeded / first / totals / emit(grid, lanes, c, a), void jobs(grid, lanes, c, a), void scan(lanes, a),
//   int read_counts(SgHead&, a)  (synchronises),  int reserve_ops(n, SgArgs&, OaArgs&)  (binds a.oa_head / a.ops and the OaArgs of the apply for n operations).
// KAI_OK: hd holds the counts, `path` the apply path that took the evictions (dry run: would take).  KAI_ERR_CAPACITY: hd.n_ops > ops_cap, nothing was applied.
template <class L>
int sg_drive(L& l, const KaiCtx& c, SgArgs& a, int lanes, bool dry_run, int64_t ops_cap, SgHead& hd, OaHead& hv, int& path) {
    path = KAI_APPLY_PATH_NONE;
    const int pod_grid = a.n_wgs, job_grid = (int)(((int64_t)c.J + lanes - 1) / lanes);
    if (pod_grid) l.succeeded(pod_grid, lanes, c, a);
    if (job_grid) l.jobs(job_grid, lanes, c, a);
    if (pod_grid) { l.first(pod_grid, lanes, c, a); l.totals(pod_grid, lanes, c, a); l.scan(lanes, a); }
    if (int rc = l.read_counts(hd, a)) return rc;
    if (hd.n_ops > ops_cap) return KAI_ERR_CAPACITY;
    if (hd.n_ops == 0) return KAI_OK;
    OaArgs oa{};
    if (int rc = l.reserve_ops(hd.n_ops, a, oa)) return rc;
    l.emit(pod_grid, lanes, c, a);
    oa.n = hd.n_ops; oa.flags = (dry_run ? (uint32_t)KAI_APPLY_CHECK_ONLY : 0u) | (oa_wide_session(c) ? 0u : KAI_OA_NOT_WIDE); oa.use_islot = oa_use_islot(c);
    const int rc = oa_drive(l, c, oa, lanes, hv, path);
    return rc == KAI_ERR_STATE ? KAI_ERR_DEVICE_FAULT : rc;  // (an evicted pod without its node: the session's own state disagrees with itself)
}

}  // namespace kai

#if defined(__HIPCC__)
namespace kai {
__global__ void __launch_bounds__(KAI_SG_WG) k_sg_succeeded(KaiCtx c, SgArgs a) { sg_succeeded_body(c, a); }
__global__ void __launch_bounds__(KAI_SG_WG) k_sg_jobs(KaiCtx c, SgArgs a) { sg_jobs_body(c, a); }
__global__ void __launch_bounds__(KAI_SG_WG) k_sg_first(KaiCtx c, SgArgs a) { sg_first_body(c, a); }
__global__ void __launch_bounds__(KAI_SG_WG) k_sg_totals(KaiCtx c, SgArgs a) { sg_totals_body(c, a); }
__global__ void __launch_bounds__(KAI_SG_WG) k_sg_scan(SgArgs a) { sg_scan_body(a); }
__global__ void __launch_bounds__(KAI_SG_WG) k_sg_emit(KaiCtx c, SgArgs a) { sg_emit_body(c, a); }
}  // namespace kai
#endif
