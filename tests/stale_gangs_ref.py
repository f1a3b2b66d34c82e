"""The stalegangeviction action restated in numpy, and the generated snapshots the stale-gang tests share.

The rules are the reference's (actions/stalegangeviction/stalegangeviction.go:29-90, api/podgroup_info/job_info.go:417-432, api/pod_status/pod_status.go:66-67); nothing here
looks at the kernels.  A job is stale when none of its pods is Succeeded, at least one is active-used and some pod-set has fewer active-used pods than its minAvailable.  A job
that is not stale loses its timestamp; a stale one keeps it, or is stamped now; when the grace period is not negative and now - stamp >= grace, every pod of the job with an
active-allocated status is evicted.  The order (ascending pod index, one `stmt` number per job with an eviction) is the library's definition (include/kai_core.h)."""
import numpy as np

import kai_testlib as T

abi = T.abi
S = abi.POD_STATUS
ACTIVE_USED = abi.ACTIVE_USED
ACTIVE_ALLOCATED = ACTIVE_USED & ~S["Releasing"]
EVICT = 2
SEC = 1_000_000_000
NOW = 1_700_000_000 * SEC
OP_DT = np.dtype([("seq", "<i8"), ("kind", "<i4"), ("pod", "<i4"), ("node", "<i4"), ("job", "<i4"), ("stmt", "<i4"), ("pad", "<i4")])
GRACES = (-1, 0, 60 * SEC)


def job_facts(snap, pod_status):
    """per job: (has a Succeeded pod, has an active-used pod, pod-sets below their minAvailable)"""
    J, NS = snap.n_jobs, snap.n_podsets
    st = np.asarray(pod_status)
    used = (st & ACTIVE_USED) != 0
    succ = np.bincount(snap.pod_job[st == S["Succeeded"]], minlength=J) > 0
    active = np.bincount(snap.pod_job[used], minlength=J) > 0
    short = np.bincount(snap.pod_podset[used], minlength=NS) < snap.podset_min_available
    n_short = np.bincount(snap.podset_job[short], minlength=J)
    return succ, active, n_short


def decide(snap, pod_status, pod_node, since, now, grace):
    """-> Result(stale, expired [J] bool; since [J]; ops: kai_op records; stale_jobs, expired_jobs)"""
    since = np.asarray(since, np.int64)
    succ, active, n_short = job_facts(snap, pod_status)
    stale = ~succ & active & (n_short > 0)
    new_since = np.where(stale, np.where(since != 0, since, now), 0).astype(np.int64)
    expired = stale & (grace >= 0) & (now - new_since >= grace)
    pods = np.nonzero(expired[snap.pod_job] & ((np.asarray(pod_status) & ACTIVE_ALLOCATED) != 0))[0]
    ops = np.zeros(len(pods), OP_DT)
    ops["seq"] = np.arange(len(pods)); ops["kind"] = EVICT; ops["pod"] = pods; ops["node"] = np.asarray(pod_node)[pods]; ops["job"] = snap.pod_job[pods]
    if len(pods):
        ops["stmt"] = np.concatenate([[0], np.cumsum(ops["job"][1:] != ops["job"][:-1])])  # a job's pods are contiguous
    return T.Result(stale=stale, expired=expired, since=new_since, ops=ops, stale_jobs=int(stale.sum()), expired_jobs=int(expired.sum()))


def categories(snap, pod_status, since, now, grace):
    """how many jobs of each kind the fuzz must contain, counted on the reference alone"""
    since = np.asarray(since, np.int64)
    st = np.asarray(pod_status)
    ref = decide(snap, st, np.zeros(snap.n_pods, np.int32), since, now, grace)
    succ, active, n_short = job_facts(snap, st)
    evictions = np.bincount(ref.ops["job"], minlength=snap.n_jobs)
    only_releasing = active & (np.bincount(snap.pod_job[(st & ACTIVE_ALLOCATED) != 0], minlength=snap.n_jobs) == 0)
    return dict(expired_with_evictions=int((ref.expired & (evictions > 0)).sum()),
                stale_inside_grace=int((ref.stale & ~ref.expired & (since != 0)).sum()),
                newly_stale=int((ref.stale & (since == 0)).sum()),
                kept_by_succeeded=int((succ & active & (n_short > 0)).sum()),
                expired_only_releasing=int((ref.expired & only_releasing).sum()),
                stale_through_one_podset=int((ref.stale & (snap.job_n_podsets > 1) & (n_short == 1)).sum()),
                recovered=int((~ref.stale & (since != 0)).sum()))


def fuzz_snapshot(seed, n_jobs=5000, pipelined=True):
    """64 nodes, about 20 000 one-GPU pods in n_jobs jobs of one to four pod-sets: job ids are a permutation of the order in which the jobs' pods lie, every 40th job has no
    pod, every status occurs (pipelined=False: no Pipelined pod, for the chip-wide apply path).  Most jobs run complete; the rest lost pods to Failed / Pending / Gated /
    Releasing, some of those also have a Succeeded pod.  -> (snap, cfg with the clock at NOW)"""
    rng = np.random.default_rng(1000 + seed)
    N, R, J = 64, 4, n_jobs
    order = rng.permutation(J)  # order[k] = the job whose pods lie k-th
    sizes = rng.choice([1, 2, 3, 4, 6, 8, 16], size=J, p=[.15, .2, .15, .2, .1, .15, .05]).astype(np.int32)
    sizes[rng.permutation(J)[: J // 40]] = 0
    n_ps = np.minimum(rng.integers(1, 5, size=J), np.maximum(sizes, 1)).astype(np.int32)
    first_ps = np.concatenate([[0], np.cumsum(n_ps)[:-1]]).astype(np.int32)
    first_pod = np.zeros(J, np.int32)
    first_pod[order] = np.concatenate([[0], np.cumsum(sizes[order])[:-1]])
    P, NS = int(sizes.sum()), int(n_ps.sum())
    pod_job = np.repeat(order, sizes[order]).astype(np.int32)
    pod_podset = np.zeros(P, np.int32); podset_min = np.ones(NS, np.int32)
    status = np.full(P, S["Running"], np.int32)
    placed = [S["Running"], S["Running"], S["Bound"], S["Binding"], S["Allocated"]] + ([S["Pipelined"]] if pipelined else [])
    gone = [S["Failed"], S["Failed"], S["Pending"], S["Gated"], S["Releasing"], S["Unknown"], S["Deleted"]]
    kind = rng.choice(5, size=J, p=[.55, .2, .1, .1, .05])  # 0 complete, 1 lost pods, 2 lost pods + Succeeded, 3 active pods all Releasing, 4 pending
    for j in range(J):
        b, n, s0, k = int(first_pod[j]), int(sizes[j]), int(first_ps[j]), int(n_ps[j])
        if n == 0: continue
        ps = np.sort(np.concatenate([np.arange(k), rng.integers(0, k, size=n - k)]))  # every pod-set has a pod
        pod_podset[b:b + n] = s0 + ps
        cnt = np.bincount(ps, minlength=k)
        podset_min[s0:s0 + k] = np.maximum(1, cnt - (rng.random(k) < 0.3))  # some pod-sets are elastic by one
        st = rng.choice(placed, size=n)
        if kind[j] in (1, 2):
            hit = rng.integers(0, k) if rng.random() < 0.6 else -1  # pods lost in exactly one pod-set, or anywhere
            lose = (ps == hit) if hit >= 0 else (rng.random(n) < 0.4)
            lose &= rng.random(n) < 0.7
            if not lose.any(): lose[rng.integers(0, n)] = True
            st[lose] = rng.choice(gone, size=int(lose.sum()))
            if kind[j] == 2: st[rng.integers(0, n)] = S["Succeeded"]
        elif kind[j] == 3:
            st[:] = S["Releasing"]; st[rng.integers(0, n)] = S["Failed"]
        elif kind[j] == 4:
            st[:] = rng.choice([S["Pending"], S["Gated"]], size=n, p=[.8, .2])
        status[b:b + n] = st
    has_node = (status & ACTIVE_USED) != 0
    pod_node = np.where(has_node, rng.integers(0, N, size=P), -1).astype(np.int32)
    alloc = np.zeros((R, N)); alloc[abi.RES_CPU] = 4_000_000.0; alloc[abi.RES_MEM] = 4096.0 * 2**30; alloc[abi.RES_GPU] = 1024; alloc[abi.RES_PODS] = 2000
    req = np.zeros((R, P)); req[abi.RES_CPU] = 1000.0; req[abi.RES_MEM] = 2.0**30; req[abi.RES_GPU] = 1.0; req[abi.RES_PODS] = 1.0
    snap = abi.Snapshot(n_res=R)
    a = snap.arrays
    a["node_allocatable"] = alloc; a["node_flags"] = np.zeros(N, np.uint32); a["node_gpu_count"] = np.full(N, 1024, np.int32); a["node_name_rank"] = rng.permutation(N).astype(np.uint32)
    a["pod_req"] = req; a["pod_job"] = pod_job; a["pod_podset"] = pod_podset; a["pod_status"] = status; a["pod_node"] = pod_node; a["pod_uid_rank"] = rng.permutation(P).astype(np.uint32)
    a["podset_job"] = np.repeat(np.arange(J, dtype=np.int32), n_ps); a["podset_min_available"] = podset_min
    a["podset_name_rank"] = (np.arange(NS) - np.repeat(first_ps, n_ps)).astype(np.uint32)
    a["job_queue"] = rng.integers(1, 5, size=J).astype(np.int32); a["job_priority"] = np.full(J, 50, np.int32); a["job_preemptible"] = (rng.random(J) < 0.8).astype(np.int32)
    a["job_created_ns"] = (rng.permutation(J).astype(np.int64) + 1) * 60 * SEC; a["job_uid_rank"] = rng.permutation(J).astype(np.uint32)
    a["job_first_pod"] = first_pod; a["job_n_pods"] = sizes; a["job_first_podset"] = first_ps; a["job_n_podsets"] = n_ps
    a["queue_parent"] = np.array([-1, 0, 0, 0, 0], np.int32); a["queue_priority"] = np.full(5, 100, np.int32); a["queue_created_ns"] = np.arange(5, dtype=np.int64) + 1
    a["queue_uid_rank"] = np.arange(5, dtype=np.uint32)
    des = np.zeros((3, 5)); des[:, 0] = [alloc[abi.RES_CPU].sum(), alloc[abi.RES_MEM].sum(), alloc[abi.RES_GPU].sum()]; des[:, 1:] = des[:, :1] / 4
    a["queue_deserved"] = des; a["queue_limit"] = np.full((3, 5), -1.0); a["queue_oqw"] = np.ones((3, 5))
    snap.finalize()
    cfg = abi.default_config()
    cfg.now_ns = NOW
    return snap, cfg


def fuzz_since(snap, seed, grace):
    """per job a timestamp from {0, now - grace - 1, now - grace, now - grace + 1} (a negative period leaves them at or behind the clock: nothing ever expires)"""
    rng = np.random.default_rng(7000 + seed)
    return rng.choice(np.array([0, NOW - grace - 1, NOW - grace, NOW - grace + 1], np.int64), size=snap.n_jobs)


def fixture_cases():
    """the reference's own table (tests/golden/stalegangeviction__stalegangeviction.json) -> [(line, snap, cfg, since, grace_ns, evictions, meta)]: a job's StaleDuration is how
    long before the clock its timestamp was set; NumberOfCacheEvictions is the expected number of evictions (0 where the case sets no mock)"""
    import json
    import os
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stalegangeviction__stalegangeviction.json")))
    out = []
    for case in doc["cases"]:
        snap, cfg, meta = T.case_to_snapshot(case)
        cfg = abi.copy_config(cfg); cfg.now_ns = NOW
        since = np.zeros(snap.n_jobs, np.int64)
        for job in case["Jobs"]:
            if job.get("StaleDuration") is not None:
                since[snap.job_names.index(job["Name"])] = NOW - int(job["StaleDuration"])
        evictions = int(((case.get("Mocks") or {}).get("CacheRequirements") or {}).get("NumberOfCacheEvictions", 0))
        out.append((case["_line"], snap, cfg, since, int(doc["staleness_grace_period_ns"]), evictions, meta))
    return out
