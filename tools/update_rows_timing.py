"""kai_session_update_rows against kai_session_open at config 5 (65 536 nodes x 1.06 M pods) on the MI355X.

  1. open S and run allocate; the next cycle's pod delta (abi.next_cycle_delta) and the rows a live cycle carries with it: the clock one minute on, every
     queue's usage, and the last start time of every job the cycle placed a pod of and of further jobs up to one row per placed pod (about 150 k);
  2. wall time in the steady state of (a) the rows alone (delta = NULL) and (b) the rows with the pod delta in one call, each against kai_session_open(S')
     in the same run: ONE session takes the change and its inverse in turn, K times each (the first update of a session is reported apart);
     the library's host clocks (KAI_PROF) split each update into staging + gather + checks, host bookkeeping and device work;
  3. the allocate that follows is hash-equal either way.

Prints one JSON line; --out writes it to a file too.  Usage: python tools/update_rows_timing.py [--scale 1.0] [--runs 7] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
from update_timing import StderrCapture, inverse, ops_hash, pkg  # noqa: E402

PROF = re.compile(r"kai update: (\d+) pods (\d+) nodes (\d+) queue rows (\d+) job rows \| stage \+ gather \+ checks ([\d.]+), host bookkeeping ([\d.]+), "
                  r"device \(scatter, classes, re-derivation\) ([\d.]+) \| total ([\d.]+) ms")


def call(lib, h, d, r):
    with StderrCapture() as cap:
        t0 = time.perf_counter(); rc = lib.kai_session_update_rows(h, None if d is None else C.byref(d), None if r is None else C.byref(r)); t1 = time.perf_counter()
    assert rc == 0, lib.kai_last_error(h)
    m = PROF.search(cap.text)
    return (t1 - t0) * 1e3, [float(m.group(k)) for k in (5, 6, 7)] if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["KAI_PROF"] = "1"
    abi = pkg.abi
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    rng = np.random.default_rng(7)
    res = {"config": desc, "pods": snap.n_pods, "nodes": snap.n_nodes, "queues": snap.n_queues, "jobs": snap.n_jobs, "runs": a.runs, "cases": []}
    equal = True
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        ops = core.open_session(snap).execute("allocate")
        delta = abi.next_cycle_delta(snap, ops, rng)
        placed = np.array([int(o["pod"]) for o in ops if int(o["kind"]) == 0], np.int64)
        jobs = np.unique(snap.pod_job[placed])
        more = np.setdiff1d(np.arange(snap.n_jobs), jobs)[: max(0, len(placed) - len(jobs))]  # ... and further jobs, up to one row per placed pod (about 150 k at full size)
        jobs = np.sort(np.concatenate([jobs, more])).astype(np.int32)
        Q = snap.n_queues
        now0 = int(cfg.now_ns)
        fw = dict(now_ns=now0 + 60 * 10**9, queues=np.arange(Q, dtype=np.int32), queue_usage=rng.random((3, Q)) * 0.9, jobs=jobs,
                  job_last_start_ns=np.full(len(jobs), now0 + 60 * 10**9, np.int64))
        old_ls = snap.arrays["job_last_start_ns"][jobs] if "job_last_start_ns" in snap.arrays else np.zeros(len(jobs), np.int64)
        bw = dict(now_ns=now0, queues=fw["queues"], queue_usage=snap.queue_usage.copy(), jobs=jobs, job_last_start_ns=old_ls)
        st_s = snap.as_struct()
        for name, d in (("rows only", None), ("rows + pod delta", delta)):
            s2, cfg2 = abi.apply_rows(snap if d is None else abi.apply_delta(snap, **d), cfg, **fw)
            st2 = s2.as_struct()
            # open(S') on a handle of cfg': the handle's clock set first (the only field of cfg' that differs)
            assert lib.kai_core_set_now(h, fw["now_ns"]) == 0
            t_open = []
            for _ in range(a.runs):
                with StderrCapture():
                    t0 = time.perf_counter(); rc = lib.kai_session_open(h, C.byref(st2)); t1 = time.perf_counter()
                assert rc == 0, lib.kai_last_error(h)
                t_open.append((t1 - t0) * 1e3)
            h_open = ops_hash(pkg.core.Session(core, s2).execute("allocate"))
            assert lib.kai_core_set_now(h, now0) == 0
            with StderrCapture():
                assert lib.kai_session_open(h, C.byref(st_s)) == 0
            dfw = dbw = None
            if d is not None:
                dfw, k1 = pkg.core.delta_struct(d["pods"], d["status"], d["node"])
                dbw, k2 = pkg.core.delta_struct(**inverse(snap, d))
            rfw, k3 = pkg.core.rows_struct(**fw)
            rbw, k4 = pkg.core.rows_struct(**bw)
            first, _ = call(lib, h, dfw, rfw)
            call(lib, h, dbw, rbw)
            walls, split = [], []
            for i in range(2 * a.runs):
                w, sp = call(lib, h, dfw if i % 2 == 0 else dbw, rfw if i % 2 == 0 else rbw)
                walls.append(w)
                if sp: split.append(sp)
            call(lib, h, dfw, rfw)
            h_upd = ops_hash(pkg.core.Session(core, s2).execute("allocate"))
            row = {"case": name, "delta_pods": 0 if d is None else len(d["pods"]), "queue_rows": int(Q), "job_rows": int(len(jobs)), "open_ms_median": statistics.median(t_open),
                   "update_ms_median": statistics.median(walls[0::2]), "update_ms_first_of_session": first, "update_ms_all": [round(x, 3) for x in walls],
                   "allocate_hash_equal": h_open == h_upd}
            sp = split[0::2]
            if sp:
                row["update_split_ms_median"] = {"stage_gather_checks": statistics.median(x[0] for x in sp), "host_bookkeeping": statistics.median(x[1] for x in sp),
                                                 "device": statistics.median(x[2] for x in sp)}
            equal = equal and h_open == h_upd
            res["cases"].append(row)
            assert lib.kai_core_set_now(h, now0) == 0
            with StderrCapture():
                assert lib.kai_session_open(h, C.byref(st_s)) == 0
    res["allocate_hash_equal"] = equal
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
