"""kai_ordered_nodes at config 5's cluster (65 536 nodes) on the MI355X, after one allocate: 1 024 pods that are still pending, over all nodes, k = 1, 8 and 64.
After the allocate config 5's cluster is full — the pending pods fit nowhere, every list is empty and nothing is ever inserted — so the same is measured on the fresh session
first, where the lists are full ("state" in each case).

Each k is timed against
  - ONE kai_best_nodes call for the same queries: the k = 1 baseline (existing code; what the scoring pass alone costs), and
  - the loop a caller has today: k kai_best_nodes calls, every query with a row of its own from which its winners so far are cleared.  A COST comparison only: under
    bin-packing that loop does not even return the same list (the pre-order range moves with the node set), so the lists are compared for k = 1 alone.
Everything goes through ctypes with arrays built beforehand; every call ends in a stream synchronise.  Each side is warmed up, then the sides alternate `--runs` times;
medians are reported.  No bar is fixed: exit status 1 only if a call fails or k = 1 differs from kai_best_nodes.

Prints one JSON line and writes it to --out (default profiles/ordered_nodes_timing_c5.json).  Usage: python tools/ordered_nodes_timing.py [--scale 1.0] [--runs 5] [--out FILE]"""
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
M_PODS, KS = 1024, (1, 8, 64)
Q_DT = np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("pad", "<i4")])
A_DT = np.dtype([("node", "<i4"), ("is_pipeline", "<i4")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_nodes_timing_c5.json"))
    a = ap.parse_args()
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    N = snap.n_nodes
    W = (N + 31) // 32
    res = {"config": desc, "nodes": N, "pods": snap.n_pods, "runs": a.runs, "cases": []}
    ok = True
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        ssn = core.open_session(snap)
        for state in ("fresh session", "after allocate"):  # the second is the state the tool is about; the first is there because a full cluster answers with empty lists
            if state == "after allocate": res["allocate_ops"] = int(len(ssn.execute("allocate")))
            ok = time_state(a, lib, h, ssn, N, W, state, res) and ok
        ssn.close()
    res["ok"] = ok
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


def time_state(a, lib, h, ssn, N, W, state, res):
    ok = True
    if True:
        st, _ = ssn.pod_states()
        pending = np.nonzero(st == abi.POD_STATUS["Pending"])[0]
        M = min(M_PODS, len(pending))
        res["queries"] = M
        q = np.zeros(M, Q_DT); q["pod"] = pending[:M]; q["nodeset"] = -1
        q_rows = q.copy(); q_rows["nodeset"] = np.arange(M)  # the removal loop: a row per query
        full = np.full((M, W), 0xffffffff, np.uint32)
        if N % 32: full[:, -1] = (1 << (N % 32)) - 1
        QP, AP, UP = C.POINTER(abi.KaiNodeQuery), C.POINTER(abi.KaiNodeAnswer), C.POINTER(C.c_uint32)

        def best(out):
            t0 = time.perf_counter()
            rc = lib.kai_best_nodes(h, q.ctypes.data_as(QP), M, None, 0, out.ctypes.data_as(AP))
            t1 = time.perf_counter()
            assert rc == 0, lib.kai_last_error(h)
            return (t1 - t0) * 1e3

        def ordered(k, out, count):
            t0 = time.perf_counter()
            rc = lib.kai_ordered_nodes(h, q.ctypes.data_as(QP), M, None, 0, k, out.ctypes.data_as(AP), count.ctypes.data_as(C.POINTER(C.c_int32)))
            t1 = time.perf_counter()
            assert rc == 0, lib.kai_last_error(h)
            return (t1 - t0) * 1e3

        def removal_loop(k, rows, out):
            """k kai_best_nodes calls; the clock sees the calls and the clearing of the winners' bits, not the reset of the rows"""
            rows[:] = full
            ans = np.zeros(M, A_DT); idx = np.arange(M)
            t0 = time.perf_counter()
            for j in range(k):
                rc = lib.kai_best_nodes(h, q_rows.ctypes.data_as(QP), M, rows.ctypes.data_as(UP), M, ans.ctypes.data_as(AP))
                assert rc == 0, lib.kai_last_error(h)
                out[:, j] = ans
                hit = ans["node"] >= 0
                n = ans["node"][hit]
                rows[idx[hit], n >> 5] &= ~(np.uint32(1) << (n & 31).astype(np.uint32))
            return (time.perf_counter() - t0) * 1e3

        a_best = np.zeros(M, A_DT)
        rows = full.copy()
        best(a_best); best(a_best)  # warm-up: code objects, the handle's scratch
        for k in KS:
            out, count, out_loop = np.zeros((M, k), A_DT), np.zeros(M, np.int32), np.zeros((M, k), A_DT)
            ordered(k, out, count); ordered(k, out, count); removal_loop(min(k, 2), rows, out_loop)
            t_best, t_ord, t_loop = [], [], []
            for r in range(a.runs):  # the sides alternate
                t_best.append(best(a_best))
                t_ord.append(ordered(k, out, count))
                if r < max(1, a.runs if k < 64 else 2): t_loop.append(removal_loop(k, rows, out_loop))
            mb, mo, ml = statistics.median(t_best), statistics.median(t_ord), statistics.median(t_loop)
            head_equal = bool(np.array_equal(out[:, 0], a_best))
            same_as_loop = float(np.mean([np.array_equal(out[i], out_loop[i]) for i in range(M)]))
            row = {"state": state, "k": k, "best_nodes_ms_median": mb, "ordered_ms_median": mo, "removal_loop_ms_median": ml, "ordered_over_best_nodes": mo / mb, "ordered_over_removal_loop": mo / ml,
                   "ordered_us_per_query": mo * 1e3 / M, "best_nodes_ms_all": [round(x, 4) for x in t_best], "ordered_ms_all": [round(x, 4) for x in t_ord],
                   "removal_loop_ms_all": [round(x, 3) for x in t_loop], "head_equals_best_nodes": head_equal, "lists_equal_to_the_removal_loop_share": same_as_loop,
                   "mean_list_length": float(count.mean()), "full_lists": int((count == k).sum())}
            ok = ok and head_equal
            res["cases"].append(row)
    return ok


if __name__ == "__main__":
    sys.exit(main())
