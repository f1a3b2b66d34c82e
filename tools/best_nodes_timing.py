"""kai_best_nodes against the loop of kai_best_node calls at config 5's cluster (65 536 nodes) on the MI355X.

After the open, for M in {1, 16, 256, 4096} pending pods of distinct jobs: the wall time of M kai_best_node calls (the only way to ask before kai_best_nodes) against ONE
kai_best_nodes call on the same handle in the same run — without a node set, and with 8 node sets of 25 % density (query i takes set i mod 8).  Both sides go through
ctypes with arguments built beforehand (bitmaps, query array), so the clock sees the library, not numpy; every call ends in a stream synchronise.  Each side is warmed
up, then the two alternate `--runs` times; medians are reported, with the time per query and the ratio batched / loop.  The answers must be equal.

The bar (from M = 256 up): the batched call's time per query under one tenth of the loop's.  Exit status 1 if it does not hold or the answers differ.

Prints one JSON line and writes it to --out (default profiles/best_nodes_timing.json).  Usage: python tools/best_nodes_timing.py [--scale 1.0] [--runs 5] [--out FILE]"""
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
SIZES = (1, 16, 256, 4096)
N_SETS, DENSITY = 8, 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_nodes_timing.json"))
    a = ap.parse_args()
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    N = snap.n_nodes
    W = (N + 31) // 32
    rng = np.random.default_rng(9)
    pending = np.nonzero(snap.pod_status == abi.POD_STATUS["Pending"])[0]
    _, first = np.unique(snap.pod_job[pending], return_index=True)  # one pending pod per job
    pods_all = pending[np.sort(first)].astype(np.int32)
    sizes = [m for m in SIZES if m <= len(pods_all)]
    words = np.zeros((N_SETS, W), np.uint32)
    for s in range(N_SETS):
        idx = np.nonzero(rng.random(N) < DENSITY)[0]
        np.bitwise_or.at(words[s], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    rows_p = [words[s].ctypes.data_as(C.POINTER(C.c_uint32)) for s in range(N_SETS)]
    res = {"config": desc, "nodes": N, "pods": snap.n_pods, "runs": a.runs, "node_sets": N_SETS, "density": DENSITY, "cases": []}
    ok = True
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        core.open_session(snap)
        node, pipe = C.c_int32(-1), C.c_int(0)

        def loop(pods, with_sets, out):
            bad = 0
            t0 = time.perf_counter()
            for i, p in enumerate(pods):
                bad |= lib.kai_best_node(h, p, rows_p[i % N_SETS] if with_sets else None, 0, C.byref(node), C.byref(pipe))
                out[i] = (node.value, pipe.value)
            t1 = time.perf_counter()
            assert bad == 0, lib.kai_last_error(h)  # the status of every call of the loop
            return (t1 - t0) * 1e3

        def batch(q, with_sets, out):
            qp, op = q.ctypes.data_as(C.POINTER(abi.KaiNodeQuery)), out.ctypes.data_as(C.POINTER(abi.KaiNodeAnswer))
            wp = words.ctypes.data_as(C.POINTER(C.c_uint32)) if with_sets else None
            t0 = time.perf_counter()
            rc = lib.kai_best_nodes(h, qp, len(q), wp, N_SETS if with_sets else 0, op)
            t1 = time.perf_counter()
            assert rc == 0, lib.kai_last_error(h)
            return (t1 - t0) * 1e3

        for with_sets in (False, True):
            for M in sizes:
                pods = [int(p) for p in pods_all[:M]]
                q = np.zeros(M, dtype=np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("pad", "<i4")]))
                q["pod"] = pods
                q["nodeset"] = np.arange(M) % N_SETS if with_sets else -1
                a_loop = np.zeros(M, dtype=np.dtype([("node", "<i4"), ("is_pipeline", "<i4")]))
                a_batch = np.zeros_like(a_loop)
                loop(pods[: min(M, 16)], with_sets, a_loop); batch(q, with_sets, a_batch); batch(q, with_sets, a_batch)  # warm-up: code objects, the handle's scratch
                t_loop, t_batch = [], []
                for _ in range(a.runs):  # the two sides alternate
                    t_loop.append(loop(pods, with_sets, a_loop))
                    t_batch.append(batch(q, with_sets, a_batch))
                same = bool(np.array_equal(a_loop, a_batch))
                ml, mb = statistics.median(t_loop), statistics.median(t_batch)
                row = {"node_sets": with_sets, "M": M, "loop_ms_median": ml, "batched_ms_median": mb, "loop_us_per_query": ml * 1e3 / M, "batched_us_per_query": mb * 1e3 / M,
                       "ratio_batched_over_loop": mb / ml, "loop_ms_all": [round(x, 3) for x in t_loop], "batched_ms_all": [round(x, 4) for x in t_batch],
                       "answers_equal": same, "fitting": int((a_batch["node"] >= 0).sum())}
                if M >= 256:
                    row["bar_under_one_tenth"] = bool(mb / ml < 0.1)
                    ok = ok and row["bar_under_one_tenth"]
                ok = ok and same
                res["cases"].append(row)
    res["ok"] = ok
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
