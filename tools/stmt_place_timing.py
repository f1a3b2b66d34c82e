"""kai_stmt_place against the composed loop of the existing calls, at config 4's full size (10 000 nodes, 13 120 topology gangs: the workload of subset_nodes_timing), on the MI355X.

On a fresh session, with the node sets and score rows of ONE kai_subset_nodes_scored call over the first 1 280 topology gangs, M = 1 / 64 / 1 024 of them (pop order is not the
subject: the first M gangs that have node sets; fewer where fewer have any: `gangs` in the JSON) are placed inside an open Statement, every gang on the first --sets-per-gang of its sets (a gang of config 4 has up to a few hundred; the call's bound
on sum n_tasks x n_sets and the rows' upload are why a caller would not send them all at once either):
 - the loop: per gang a checkpoint, per set and task kai_ordered_nodes_scored(k = 1) and kai_stmt_apply of one operation, kai_stmt_rollback of a set that fails — the ctypes
   calls of a Python loop, a host clock around the whole loop.  With --loop-lib it runs in a child process on ANOTHER build of the library (the parent commit's);
 - one kai_stmt_place call: a host clock around the call (it ends in a stream synchronise), after one warm-up call that grows the handle's scratch.
Between two runs the Statement is discarded, so every run starts from the fresh state.  Before anything is timed the operations and the three read-backs of the two are
compared: they must be equal.  Medians of --runs.  No bar is set: every figure is written down.
 - the kernels' own time: a child process of its own with KAI_PLACE_PROF=1 (the library waits for every launch between two events and prints the milliseconds of k_sp_prep
   and k_sp_place), one warm-up and one call per M, so that the end-to-end figures above are taken without it.
NOTE on the workload: --sets-per-gang truncates every gang's set list; a gang that none of its first sets takes is NO_FIT here where the full walk would go on.  The JSON
says so (`sets_note`).

Prints one JSON line and writes it to --out (default profiles/stmt_place_timing_c4.json).
Usage: python tools/stmt_place_timing.py [--scale 1.0] [--runs 5] [--sets-per-gang 4] [--loop-lib FILE] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COUNTS = (1, 64, 1024)
Q_DT = np.dtype([("job", "<i4"), ("group", "<i4"), ("podset", "<i4"), ("nodeset", "<i4")])
A_DT = np.dtype([("status", "<i4"), ("n_sets", "<i4"), ("first", "<i4"), ("tasks", "<i4"), ("common_domain", "<i4"), ("pad", "<i4")])
G_DT = np.dtype([("first_task", "<i4"), ("n_tasks", "<i4"), ("first_set", "<i4"), ("n_sets", "<i4"), ("scores", "<i4"), ("pad", "<i4")])
PA_DT = np.dtype([("status", "<i4"), ("set", "<i4"), ("sets_tried", "<i4"), ("pad", "<i4"), ("first_op", "<i8"), ("n_ops", "<i8")])
SQ_DT = np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("scores", "<i4")])
NA_DT = np.dtype([("node", "<i4"), ("is_pipeline", "<i4")])


def load_pkg(lib_path):
    """the package on the repository's own library, or — lib_path — on another build of it that may lack the newest entry points: only what this tool calls is declared"""
    import __graft_entry__ as entry
    pkg = entry._load_pkg()
    if lib_path:
        abi = pkg.abi
        lib = C.CDLL(lib_path)
        lib.kai_last_error.restype = C.c_char_p; lib.kai_last_error.argtypes = [C.c_void_p]; lib.kai_version.restype = C.c_char_p
        lib.kai_core_create.argtypes = [C.POINTER(abi.KaiConfig), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        lib.kai_core_destroy.argtypes = [C.c_void_p]; lib.kai_session_close.argtypes = [C.c_void_p]
        lib.kai_session_open.argtypes = [C.c_void_p, C.POINTER(abi.KaiSnapshotSoA)]
        lib.kai_queue_shares.argtypes = [C.c_void_p, C.POINTER(abi.KaiQueueShare), C.c_int]
        lib.kai_pod_states.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
        lib.kai_node_states.argtypes = [C.c_void_p, C.POINTER(abi.KaiNodeState), C.c_int]
        lib.kai_stmt_begin.argtypes = [C.c_void_p, C.c_uint32]; lib.kai_stmt_checkpoint.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.kai_stmt_rollback.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(abi.KaiStmtResult)]; lib.kai_stmt_discard.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.KaiStmtResult)]
        pkg.core._lib = lib
    return pkg


def digest(ssn):
    h = hashlib.sha256()
    st, nd = ssn.pod_states(); h.update(st.tobytes()); h.update(nd.tobytes())
    ns = ssn.node_states(); [h.update(np.ascontiguousarray(ns[k]).tobytes()) for k in ("idle", "releasing", "used")]
    qs = ssn.queue_shares(); [h.update(np.ascontiguousarray(qs[k]).tobytes()) for k in sorted(qs)]
    return h.hexdigest()


class Case:
    """config 4's session, the sets of its topology gangs (one scored subset call, direct: the wrapper's boolean masks of 170 000 sets would not fit), the place data per M"""

    def __init__(self, pkg, scale, sets_per_gang):
        self.pkg, self.abi = pkg, pkg.abi
        abi = pkg.abi
        self.snap, self.cfg, self.desc = pkg.synth.config(3, scale)
        a = self.snap.arrays
        self.jobs = np.nonzero(a["group_topology"][a["job_root_group"]] >= 0)[0].astype(np.int32)
        self.core = pkg.KaiCore(self.cfg); self.ssn = self.core.open_session(self.snap)
        self.lib, self.h = self.core.lib, self.core.handle.value
        self.lib.kai_subset_nodes_scored.argtypes = None; self.lib.kai_ordered_nodes_scored.argtypes = None; self.lib.kai_stmt_apply.argtypes = None
        self.N = self.snap.n_nodes; self.W = (self.N + 31) // 32
        self.D = int(a["domain_level"].shape[0])
        want = min(len(self.jobs), max(COUNTS) + 256)
        jobs = self.jobs[:want]
        q = np.zeros(len(jobs), Q_DT); q["job"] = jobs; q["group"] = -1; q["podset"] = -1; q["nodeset"] = -1
        ans = np.zeros(len(jobs), A_DT); pm = abi.KaiSubsetParams(abi.SUBSET_VERSION, 0); n = C.c_int64(0); res = abi.KaiSubsetResult()
        self.score_rows = np.zeros(len(jobs), np.dtype([("level_row", "<i4"), ("n_scored", "<i4")])); self.deciles = np.zeros((len(jobs), max(self.D, 1)), np.uint8)
        cap = 64
        for _ in range(2):
            sets = np.zeros(cap * 4, np.int32); maps = np.zeros(cap * self.W, np.uint32)
            rc = self.lib.kai_subset_nodes_scored(C.c_void_p(self.h), C.byref(pm), C.c_void_p(q.ctypes.data), C.c_int32(len(q)), None, C.c_int32(0), C.c_void_p(ans.ctypes.data), C.c_void_p(sets.ctypes.data),
                                                  C.c_int64(cap), C.byref(n), C.c_void_p(maps.ctypes.data), C.c_void_p(self.score_rows.ctypes.data), C.c_void_p(self.deciles.ctypes.data), C.byref(res))
            if rc != -4: break
            cap = int(n.value)
        assert rc == 0, (rc, self.lib.kai_last_error(C.c_void_p(self.h)))
        maps = maps.reshape(cap, self.W)
        pend = a["pod_status"] == abi.POD_STATUS["Pending"]
        self.gangs = []  # (query index, pods, rows of `maps`)
        for i, j in enumerate(jobs):
            if ans["status"][i] != 0 or ans["n_sets"][i] < 1: continue
            pods = np.nonzero((a["pod_job"] == j) & pend)[0].astype(np.int32) if len(self.gangs) < max(COUNTS) else None
            if pods is None: break
            if len(pods): self.gangs.append((i, pods, list(range(int(ans["first"][i]), int(ans["first"][i]) + min(int(ans["n_sets"][i]), sets_per_gang)))))
        self.maps = maps

    def data(self, m):
        """the arrays of one call for the first m gangs: only the rows they name, renumbered"""
        gs = self.gangs[:m]
        gv = np.zeros(len(gs), G_DT); tasks, sets, rows = [], [], []
        for g, (i, pods, rr) in enumerate(gs):
            gv[g] = (len(tasks), len(pods), len(sets), len(rr), i, 0)
            tasks += pods.tolist(); sets += list(range(len(rows), len(rows) + len(rr))); rows += rr
        return gv, np.array(tasks, np.int32), np.array(sets, np.int32), np.ascontiguousarray(self.maps[rows])

    def place(self, d, runs):
        abi = self.abi
        gv, tasks, sets, words = d
        ans = np.zeros(len(gv), PA_DT); fail = np.zeros(len(sets), np.int32); ops = np.zeros(len(tasks), self.pkg.core._OP_DTYPE); n = C.c_int64(0); res = abi.KaiStmtResult()
        pm = abi.KaiPlaceParams(abi.PLACE_VERSION, 0)
        ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        ms = []
        for r in range(runs + 1):  # (the first run warms the handle's scratch)
            t = self.ssn.statement()
            t0 = time.perf_counter()
            rc = self.lib.kai_stmt_place(C.c_void_p(self.h), C.byref(pm), gv.ctypes.data_as(C.POINTER(abi.KaiPlaceGang)), len(gv), ip(tasks), len(tasks), ip(sets), len(sets),
                                         words.ctypes.data_as(C.POINTER(C.c_uint32)), len(words), self.score_rows.ctypes.data_as(C.POINTER(abi.KaiTopoScoreRow)),
                                         self.deciles.ctypes.data_as(C.POINTER(C.c_uint8)), len(self.score_rows), ans.ctypes.data_as(C.POINTER(abi.KaiPlaceAnswer)), ip(fail),
                                         ops.ctypes.data_as(C.POINTER(abi.KaiOp)), len(ops), C.byref(n), C.byref(res))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0, (rc, self.lib.kai_last_error(C.c_void_p(self.h)))
            out = [(int(o["kind"]), int(o["pod"]), int(o["node"])) for o in ops[: n.value]]
            state = digest(self.ssn) if r == 0 else None
            t.discard()
            if r == 0: first = (out, state, int(res.path), int((ans["status"] == 0).sum()))
        return ms[1:], first

    def loop(self, d, runs):
        abi = self.abi
        gv, tasks, sets, words = d
        q = np.zeros(1, SQ_DT); out = np.zeros(1, NA_DT); cnt = np.zeros(1, np.int32); op = np.zeros(1, self.pkg.core._OP_DTYPE); res = abi.KaiStmtResult()
        lib, h = self.lib, C.c_void_p(self.h)
        sr, dc, n_sr = C.c_void_p(self.score_rows.ctypes.data), C.c_void_p(self.deciles.ctypes.data), C.c_int32(len(self.score_rows))
        qp, outp, cntp, opp = C.c_void_p(q.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(cnt.ctypes.data), C.c_void_p(op.ctypes.data)
        ms = []
        for r in range(runs + 1):
            t = self.ssn.statement()
            done = []
            t0 = time.perf_counter()
            for g in gv:
                cp = t.checkpoint()
                for si in range(g["first_set"], g["first_set"] + g["n_sets"]):
                    row = C.c_void_p(words[sets[si]].ctypes.data)
                    ok = True
                    for p in tasks[g["first_task"]: g["first_task"] + g["n_tasks"]]:
                        q[0] = (p, 0, 0, g["scores"])
                        rc = lib.kai_ordered_nodes_scored(h, qp, C.c_int32(1), row, C.c_int32(1), sr, dc, n_sr, C.c_int32(1), outp, cntp)
                        assert rc == 0, (rc, lib.kai_last_error(C.c_void_p(self.h)))
                        if cnt[0] < 1: ok = False; break
                        op[0]["kind"], op[0]["pod"], op[0]["node"] = (1 if out[0]["is_pipeline"] else 0), p, out[0]["node"]
                        rc = lib.kai_stmt_apply(h, opp, C.c_int64(1), C.c_uint32(0), C.byref(res))
                        assert rc == 0, (rc, lib.kai_last_error(C.c_void_p(self.h)))
                        done.append((int(op[0]["kind"]), int(p), int(out[0]["node"])))
                    if ok: break
                    t.rollback(cp); del done[cp:]
            ms.append((time.perf_counter() - t0) * 1e3)
            state = digest(self.ssn) if r == 0 else None
            t.discard()
            if r == 0: first = (done, state)
        return ms[1:], first

    def close(self):
        self.ssn.close(); self.core.destroy()


def loop_child(a):
    pkg = load_pkg(a.loop_lib)
    case = Case(pkg, a.scale, a.sets_per_gang)
    out = {}
    for m in COUNTS:
        ms, first = case.loop(case.data(m), a.runs)
        out[str(m)] = dict(ms=[round(x, 3) for x in ms], ops=first[0], state=first[1])
    case.close()
    print(json.dumps(dict(version=pkg.core.load_library().kai_version().decode(), counts=out)))
    return 0


def prof_child(a):
    """one warm-up and one call per M under KAI_PLACE_PROF (set by the parent): the library prints the split"""
    pkg = load_pkg("")
    case = Case(pkg, a.scale, a.sets_per_gang)
    for m in COUNTS:
        sys.stderr.write(f"kai stmt place M {m}\n"); sys.stderr.flush()
        case.place(case.data(m), 1)
    case.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sets-per-gang", type=int, default=4)
    ap.add_argument("--loop-lib", default="", help="another build of libkai_core.so for the loop (the parent commit's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stmt_place_timing_c4.json"))
    ap.add_argument("--loop-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--prof-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop_child: return loop_child(a)
    if a.prof_child: return prof_child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--loop-child", "--scale", str(a.scale), "--runs", str(a.runs), "--sets-per-gang", str(a.sets_per_gang)] + (["--loop-lib", a.loop_lib] if a.loop_lib else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    base = json.loads(p.stdout.strip().splitlines()[-1])
    pp = subprocess.run([sys.executable, os.path.abspath(__file__), "--prof-child", "--scale", str(a.scale), "--sets-per-gang", str(a.sets_per_gang)], capture_output=True, text=True,
                        env=dict(os.environ, KAI_PLACE_PROF="1"))
    assert pp.returncode == 0, pp.stderr[-3000:]
    split, cur = {}, None
    for ln in pp.stderr.splitlines():
        if ln.startswith("kai stmt place M "): cur = ln.split()[-1]
        elif ln.startswith("kai stmt place: ") and cur is not None:
            w = ln.split("|")[1].split(); split[cur] = {w[0]: float(w[1]), w[2]: float(w[3])}  # (the last line of an M: the call behind the warm-up)
    pkg = load_pkg("")
    case = Case(pkg, a.scale, a.sets_per_gang)
    out = dict(sets_note=f"every gang is placed on the first {a.sets_per_gang} of its node sets only (kai_subset_nodes_scored gives a gang of this workload up to a few hundred): not the full allocatePodSet walk",
               scale=a.scale, runs=a.runs, sets_per_gang=a.sets_per_gang, config=case.desc, nodes=case.snap.n_nodes, pods=case.snap.n_pods, topology_gangs=int(len(case.jobs)),
               loop_library=base["version"] + (" (--loop-lib)" if a.loop_lib else ""), library=pkg.core.load_library().kai_version().decode(), counts={})
    for m in COUNTS:
        d = case.data(m)
        ms, first = case.place(d, a.runs)
        b = base["counts"][str(m)]
        equal = [list(x) for x in first[0]] == [list(x) for x in b["ops"]] and first[1] == b["state"]
        assert equal, f"M = {m}: the call and the loop differ (operations {len(first[0])} / {len(b['ops'])}, read-backs {first[1][:12]} / {b['state'][:12]})"
        out["counts"][str(m)] = dict(gangs=len(d[0]), tasks=int(len(d[1])), tasks_per_gang=round(len(d[1]) / max(len(d[0]), 1), 2), sets=int(len(d[2])), placed_gangs=first[3], operations=len(first[0]),
                                     path={1: "wide", 2: "engine"}.get(first[2], "none"), equal_operations_and_read_backs=True,
                                     loop_ms=b["ms"], loop_median_ms=round(statistics.median(b["ms"]), 3), place_ms=[round(x, 3) for x in ms], place_median_ms=round(statistics.median(ms), 3),
                                     loop_over_place=round(statistics.median(b["ms"]) / statistics.median(ms), 1), kernel_ms=split.get(str(m)),
                                     kernel_sum_ms=round(sum(split[str(m)].values()), 4) if str(m) in split else None)
    case.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f: f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
