"""kai_stale_gang_eviction at config 5's full size on the MI355X.

The session: config 5 after one allocate; then, by kai_session_update, the placed pods are Running on their nodes and about 1 % of the running gangs (jobs of two or more
pods, all placed) lose one pod to Failed.  Every job carries a staleness timestamp one nanosecond past the grace period, so every stale gang is evicted.

 - the call: median over --runs (each run: the same kai_session_update again, which restores the session, then ONE kai_stale_gang_eviction through ctypes; the call ends in
   a stream synchronise), after one warm-up call that grows the handle's scratch;
 - beside it, what a caller does today on the same session: kai_pod_states, the decision in numpy (the rules of include/kai_core.h), kai_ops_apply of the evictions.
Both must produce the same operations and leave the same pod states.  No bar is set: both figures and the launch count are written down.

One process.  Prints one JSON line and writes it to --out (default profiles/stale_gangs_timing_c5.json).  Usage: python tools/stale_gangs_timing.py [--scale 1.0] [--runs 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry._load_pkg()
abi = pkg.abi
S = abi.POD_STATUS
SEC = 1_000_000_000
NOW, GRACE = 1_700_000_000 * SEC, 60 * SEC
ACTIVE_ALLOCATED = abi.ACTIVE_USED & ~S["Releasing"]
OP_DT = pkg.core._OP_DTYPE


def decide(snap, st, nd, since, now, grace):
    """the action's rules in numpy -> (evictions as kai_op records, new timestamps, Stale)"""
    J, NS = snap.n_jobs, snap.n_podsets
    used = (st & abi.ACTIVE_USED) != 0
    succ = np.bincount(snap.pod_job[st == S["Succeeded"]], minlength=J) > 0
    active = np.bincount(snap.pod_job[used], minlength=J) > 0
    short = np.bincount(snap.pod_podset[used], minlength=NS) < snap.podset_min_available
    stale = ~succ & active & (np.bincount(snap.podset_job[short], minlength=J) > 0)
    new_since = np.where(stale, np.where(since != 0, since, now), 0)
    expired = stale & (grace >= 0) & (now - new_since >= grace)
    pods = np.nonzero(expired[snap.pod_job] & ((st & ACTIVE_ALLOCATED) != 0))[0]
    ops = np.zeros(len(pods), OP_DT)
    ops["seq"] = np.arange(len(pods)); ops["kind"] = 2; ops["pod"] = pods; ops["node"] = nd[pods]; ops["job"] = snap.pod_job[pods]
    if len(pods): ops["stmt"] = np.concatenate([[0], np.cumsum(ops["job"][1:] != ops["job"][:-1])])
    return ops, new_since, expired


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stale_gangs_timing_c5.json"))
    a = ap.parse_args()
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    cfg = abi.copy_config(cfg); cfg.now_ns = NOW
    out = dict(config=desc, scale=a.scale, nodes=snap.n_nodes, pods=snap.n_pods, jobs=snap.n_jobs, runs=a.runs, grace_s=GRACE // SEC)
    rng = np.random.default_rng(5)
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        ssn = core.open_session(snap)
        placed = ssn.execute("allocate")
        st, nd = ssn.pod_states()
        st, nd = st.copy(), nd.copy()
        on = (st & ACTIVE_ALLOCATED) != 0
        whole = (np.bincount(snap.pod_job[on], minlength=snap.n_jobs) == snap.job_n_pods) & (snap.job_n_pods >= 2)  # running gangs
        gangs = np.nonzero(whole)[0]
        losers = rng.choice(gangs, size=max(1, len(gangs) // 100), replace=False)
        lost = (snap.job_first_pod[losers] + rng.integers(0, snap.job_n_pods[losers])).astype(np.int32)
        pods = np.unique(np.concatenate([placed["pod"].astype(np.int32), lost]))
        status = np.where(np.isin(pods, lost), S["Failed"], S["Running"]).astype(np.int32)
        node = np.where(np.isin(pods, lost), -1, nd[pods]).astype(np.int32)
        d, keep = pkg.core.delta_struct(pods, status, node)
        since0 = np.full(snap.n_jobs, NOW - GRACE - 1, np.int64)
        out["running_gangs"] = int(len(gangs)); out["gangs_that_lost_a_pod"] = int(len(losers))

        def restore():
            rc = lib.kai_session_update(h, C.byref(d))
            assert rc == 0, (rc, lib.kai_last_error(h))

        P, J = snap.n_pods, snap.n_jobs
        ops_buf = np.zeros(P, OP_DT); stale = np.zeros(J, np.uint8); n = C.c_int64(0); res = abi.KaiStaleResult()
        params = abi.KaiStaleParams(abi.STALE_VERSION, 0, GRACE)

        def call():
            restore()
            since = since0.copy()
            t0 = time.perf_counter()
            rc = lib.kai_stale_gang_eviction(h, C.byref(params), since.ctypes.data_as(C.POINTER(C.c_int64)), stale.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             ops_buf.ctypes.data_as(C.POINTER(abi.KaiOp)), P, C.byref(n), C.byref(res))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, lib.kai_last_error(h))
            return ms, ops_buf[: n.value].copy(), since, stale.astype(bool), ssn.pod_states()

        def today():
            restore()
            st_b, nd_b = np.zeros(P, np.int32), np.zeros(P, np.int32); ares = abi.KaiApplyResult()
            t0 = time.perf_counter()
            rc = lib.kai_pod_states(h, st_b.ctypes.data_as(C.POINTER(C.c_int32)), nd_b.ctypes.data_as(C.POINTER(C.c_int32)), P)
            t1 = time.perf_counter()
            ops, since, expired = decide(snap, st_b, nd_b, since0, NOW, GRACE)
            t2 = time.perf_counter()
            rc2 = lib.kai_ops_apply(h, ops.ctypes.data_as(C.POINTER(abi.KaiOp)), len(ops), 0, C.byref(ares))
            t3 = time.perf_counter()
            assert rc == 0 and rc2 == 0, (rc, rc2, lib.kai_last_error(h))
            return ((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), ops, since, expired, ssn.pod_states(), ares.path

        call(); today()  # warm-up: the handle's scratch and staging grow here
        calls = [call() for _ in range(a.runs)]
        todays = [today() for _ in range(a.runs)]
        _, ops, since, expired, (st_a, nd_a) = calls[-1]
        _, ops_t, since_t, expired_t, (st_t, nd_t), path_t = todays[-1]
        assert len(ops) > 0 and ops.tobytes() == ops_t.tobytes(), "the call and the caller's own decision produce different operations"
        assert np.array_equal(since, since_t) and np.array_equal(expired, expired_t) and (st_a == st_t).all() and (nd_a == nd_t).all()
        assert res.path == path_t
        out["stale_jobs"] = int(res.stale_jobs); out["expired_jobs"] = int(res.expired_jobs); out["evictions"] = int(len(ops))
        out["apply_path"] = {abi.APPLY_PATH_WIDE: "wide", abi.APPLY_PATH_ENGINE: "engine"}.get(res.path, str(res.path))
        out["launches"] = 8 if res.path == abi.APPLY_PATH_WIDE else 9  # Succeeded flags, jobs, first pods, totals, their scan, emit, the apply's check and chip-wide pass (+ the engine walk)
        out["call_ms"] = [round(c[0], 3) for c in calls]; out["call_median_ms"] = round(statistics.median(c[0] for c in calls), 3)
        out["today_ms"] = [round(t[0][0], 3) for t in todays]; out["today_median_ms"] = round(statistics.median(t[0][0] for t in todays), 3)
        for i, k in enumerate(("pod_states", "numpy_decision", "ops_apply")):
            out[f"today_{k}_median_ms"] = round(statistics.median(t[0][i + 1] for t in todays), 3)
        ssn.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
