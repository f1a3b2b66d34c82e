// kai_delta.hpp — kernels of kai_session_update / kai_session_update_rows (include/kai_core.h): a pod / node delta, and the queue rows and job start times that change
// between two cycles, applied to the HBM-resident snapshot of an open session.
//
// The host stages the delta in ONE pinned buffer and sends it with one copy (DeltaView: the arrays inside that buffer).  k_delta_gather reads what the
// snapshot holds for every changed pod (status, node, shared-GPU group, flags) without writing the session, so that every refusal is decided before the
// first write; it also adds up the delta's effect on the count of Releasing / Pipelined pods (wavefront reductions, one atomic per workgroup; the host
// adjusts the pending pods per request key itself, from the old statuses gathered here).  k_apply_delta then
// scatters the delta into the baselines kai_session_reset restores (d_status0 / d_node0 / aux.group0) and into the nodes' allocatable rows and flags,
// mapping the caller's node indices through the name-rank permutation.  k_class_remap re-labels every pod's scan class when the class table changed.
// k_apply_rows scatters the rows (RowsView: further arrays of the same buffer) into the QShare baseline, the queues' priorities and min-runtime settings and the jobs'
// last start times; nothing on the host or the device is derived from those except what kai_session_reset's kernels compute again after every scatter.
// The CPU suite runs none of these kernels (its stand-in runtime launches nothing, the emulator does not take them): tests/test_gpu_update_chains.py holds them, and the
// host's bookkeeping around them, to a fresh open across chains of updates (tests/update_chains.py), at delta sizes on both sides of a workgroup's 256 threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kai_engine.hpp"

namespace kai {

constexpr int KD_TB = 256;        // threads per workgroup of the delta kernels (4 wavefronts)
constexpr int KD_KEEP = INT32_MIN;  // a group entry the delta leaves unchanged
constexpr int KD_NCNT = 1;        // per-session counters adjusted by a delta: [0] Releasing or Pipelined pods

// The delta as it sits in the staging buffer (device addresses of the one upload).  Pod entries: index, new status, new node (caller's index or -1),
// new group (KD_KEEP = unchanged; the host has already applied the open's rule "a group only on a shared-GPU request").  Node entries: index (caller's),
// new flags (already masked to the public bits, the library's own bits merged back by the host), new allocatable [R][n_nodes].
struct DeltaView {
    const int32_t* pod; const int32_t* pod_status; const int32_t* pod_node; const int32_t* pod_group;
    const int32_t* node; const uint32_t* node_flags; const double* node_alloc;
    int32_t n_pods, n_nodes, R, N;
    const uint32_t* rank;  // [N] node_name_rank: caller's node index -> engine index
};

// Where the parts of one update lie in its staging buffer (the pinned and the device copy alike), every part on a 256-byte boundary: [pod | status | node | group | node |
// flags] int32, [R][NNcap] doubles, the rows ([queue | priority | job] int32, then 8-byte values: deserved, limit, oqw, usage [3][NQ] each, the two min-runtimes [NQ] each,
// last start [NJ]); behind what is sent, the gather's output [4][NP] int32 and its counters.
struct DeltaLayout {
    int NNcap;  // node entries: the delta's, and the nodes whose legacy-MIG bit a pod of the delta changes
    size_t o_i32 = 0, o_f64, o_r32, o_r64, o_out, o_cnt, total;
    static size_t up8(size_t b) { return (b + 255) & ~(size_t)255; }
    DeltaLayout(int NP, int NN, int R, int NQ, int NJ, bool legacy_mig) : NNcap(NN + (legacy_mig ? 2 * NP : 0)) {
        o_f64 = up8(((size_t)4 * NP + 2 * NNcap) * 4); o_r32 = up8(o_f64 + (size_t)R * NNcap * 8); o_r64 = up8(o_r32 + ((size_t)2 * NQ + NJ) * 4);
        o_out = up8(o_r64 + ((size_t)14 * NQ + NJ) * 8); o_cnt = up8(o_out + (size_t)4 * NP * 4); total = o_cnt + 256;
    }
};

__device__ __forceinline__ int kd_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Read-only: what the session's snapshot holds for each changed pod, and the counter adjustments old -> new.
__global__ void __launch_bounds__(KD_TB) k_delta_gather(DeltaView d, const int32_t* __restrict__ status0, const int32_t* __restrict__ node0, const int32_t* __restrict__ group0,
                                                        const uint32_t* __restrict__ flags, int32_t* __restrict__ out, int32_t* __restrict__ counters) {
    __shared__ int part[KD_TB / 64][KD_NCNT];
    const int i = blockIdx.x * KD_TB + threadIdx.x;
    int drel = 0;
    if (i < d.n_pods) {
        const int p = d.pod[i];
        const int so = status0[p], sn = d.pod_status[i];
        out[i] = so; out[d.n_pods + i] = node0[p]; out[2 * d.n_pods + i] = group0[p]; out[3 * d.n_pods + i] = (int32_t)flags[p];
        const int rp = KAI_POD_RELEASING | KAI_POD_PIPELINED;
        drel = ((sn & rp) ? 1 : 0) - ((so & rp) ? 1 : 0);
    }
    drel = kd_wave_sum(drel);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) part[w][0] = drel;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int k = 0; k < KD_TB / 64; k++) a += part[k][0];
        if (a) atomicAdd(&counters[0], a);
    }
}

// The scatter: one thread per changed pod, then one per changed node (every index was range-checked by the host).
__global__ void __launch_bounds__(KD_TB) k_apply_delta(DeltaView d, int32_t* __restrict__ status0, int32_t* __restrict__ node0, int32_t* __restrict__ group0,
                                                       double* __restrict__ n_alloc, uint32_t* __restrict__ n_flags) {
    const int i = blockIdx.x * KD_TB + threadIdx.x;
    if (i < d.n_pods) {
        const int p = d.pod[i], n = d.pod_node[i];
        status0[p] = d.pod_status[i];
        node0[p] = n >= 0 ? (int32_t)d.rank[n] : -1;
        if (d.pod_group[i] != KD_KEEP) group0[p] = d.pod_group[i];
    } else if (i < d.n_pods + d.n_nodes) {
        const int k = i - d.n_pods, e = (int)d.rank[d.node[k]];
        n_flags[e] = d.node_flags[k];
        for (int r = 0; r < d.R; r++) n_alloc[(size_t)r * d.N + e] = d.node_alloc[(size_t)r * d.n_nodes + k];
    }
}

// The rows of kai_session_update_rows as they sit in the same staging buffer, behind the pod / node delta (one upload for both).  A quantity the call leaves
// unchanged is a null pointer here; the index arrays were range-checked by the host and hold no index twice.
struct RowsView {
    const int32_t* queue; const double* deserved; const double* limit; const double* oqw; const double* usage;  // [n_queues]; the four quantities [3][n_queues], units of the snapshot's
    const int32_t* prio; const int64_t* preempt_mr; const int64_t* reclaim_mr;
    const int32_t* job; const int64_t* last_start;  // [n_jobs]
    int32_t n_queues, n_jobs;
};

// A queue's deserved / limit value of resource k as the open stores it (HostPrep::build, proportion.createQueueResourceAttrs): memory in bytes, "unlimited" kept.
// One multiplication and one compare, the same on the host and on the device: a row written here equals the one an open builds bit for bit.
KAI_HD double kd_quota_row(int k, double v) {
    if (k != KAI_Q_MEM) return v;
    const double x = v * 1000000.0;
    return KAI_UNLIMITED < x ? x : KAI_UNLIMITED;
}

// The scatter of the rows: one thread per changed queue writes its rows into the QShare baseline kai_session_reset restores (q * 3 + k), its priority and its
// min-runtime settings; behind the queues one thread per changed job writes its last start time.
__global__ void __launch_bounds__(KD_TB) k_apply_rows(RowsView v, QShare* __restrict__ shares0, int32_t* __restrict__ q_prio, int64_t* __restrict__ q_preempt_mr,
                                                      int64_t* __restrict__ q_reclaim_mr, int64_t* __restrict__ j_last_start) {
    const int i = blockIdx.x * KD_TB + threadIdx.x;
    if (i < v.n_queues) {
        const int q = v.queue[i];
        for (int k = 0; k < 3; k++) {
            QShare& x = shares0[(size_t)q * 3 + k]; const size_t at = (size_t)k * v.n_queues + i;
            if (v.deserved) x.deserved = kd_quota_row(k, v.deserved[at]);
            if (v.limit) x.max_allowed = kd_quota_row(k, v.limit[at]);
            if (v.oqw) x.oqw = v.oqw[at];
            if (v.usage) x.usage = v.usage[at];
        }
        if (v.prio) q_prio[q] = v.prio[i];
        if (v.preempt_mr) q_preempt_mr[q] = v.preempt_mr[i];
        if (v.reclaim_mr) q_reclaim_mr[q] = v.reclaim_mr[i];
    } else if (i < v.n_queues + v.n_jobs) {
        const int k = i - v.n_queues;
        if (v.last_start) j_last_start[v.job[k]] = v.last_start[k];
    }
}

// Every pod's scan class from its request key (a new class table: kai_host_prep.hpp rank_classes); a shared-GPU request is in no class.
__global__ void __launch_bounds__(KD_TB) k_class_remap(int P, const int32_t* __restrict__ pod_key, const uint8_t* __restrict__ shared, int shared_on, const int32_t* __restrict__ remap,
                                                       int32_t* __restrict__ scls) {
    const int p = blockIdx.x * KD_TB + threadIdx.x;
    if (p < P) scls[p] = (shared_on && shared[p]) ? -1 : remap[pod_key[p]];
}

}  // namespace kai
