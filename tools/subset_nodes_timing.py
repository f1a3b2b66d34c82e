"""kai_subset_nodes at config 4's full size (10 000 nodes, 8 zones x 40 racks) and on mixed config 5, on the MI355X.

Per configuration two sessions of one handle: as opened ("fresh") and after one allocate ("after_allocate").  On each, for M = 1, 64 and 1 024 queried topology gangs (the
root sub-group sets of the jobs that carry a constraint, cycled where the session has fewer):
 - the chip-wide path: median over --runs calls through ctypes (a host clock around a call that ends in a stream synchronise), after one warm-up call that grows the
   handle's scratch;
 - the engine path (KAI_SUBSET_ENGINE_PATH) on the same queries, with the same answers required.  One lane walks one query after the other: where the time per query
   of a smaller M says that a call would take more than --engine-cap-s seconds, it is skipped and the estimate is written down instead;
 - the loop of M one-query calls on the chip-wide path (what a caller pays who asks per gang);
 - the per-launch split of the chip-wide path: a child process of its own with KAI_SUBSET_PROF=1 (the library waits for every launch between two events and prints the
   milliseconds per kernel), so that the end-to-end figures above are taken without it.
No bar is set: every figure is written down.

Prints one JSON line and writes it to --out (default profiles/subset_nodes_timing_c4.json).
Usage: python tools/subset_nodes_timing.py [--scale 1.0] [--runs 7] [--engine-cap-s 20] [--configs 3,4m] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry._load_pkg()
abi = pkg.abi
PATHS = {abi.SUBSET_PATH_NONE: "none", abi.SUBSET_PATH_WIDE: "wide", abi.SUBSET_PATH_ENGINE: "engine"}
COUNTS = (1, 64, 1024)
Q_DT = np.dtype([("job", "<i4"), ("group", "<i4"), ("podset", "<i4"), ("nodeset", "<i4")])


def load(key, scale):
    """"3" = config 4, "4m" = mixed config 5 -> (snapshot, config, description, the jobs whose root group carries a topology constraint)"""
    snap, cfg, desc = pkg.synth.config(int(key.rstrip("m")), scale, mixed=key.endswith("m"))
    a = snap.arrays
    jobs = np.nonzero(a["group_topology"][a["job_root_group"]] >= 0)[0].astype(np.int32) if "group_topology" in a else np.zeros(0, np.int32)
    return snap, cfg, desc, jobs


class Caller:
    MAP_BYTES_MAX = 1 << 30  # above this the bitmap rows of a call are not asked for (written down as "bitmaps": false)

    def __init__(self, core, snap):
        self.lib, self.h, self.W = core.lib, core.handle, max((snap.n_nodes + 31) // 32, 1)
        self.n, self.res = C.c_int64(0), abi.KaiSubsetResult()
        self.room(64)

    def room(self, cap):
        self.cap = cap
        self.with_maps = cap * self.W * 4 <= self.MAP_BYTES_MAX
        self.sets = np.zeros(cap * 4, np.int32); self.maps = np.zeros(cap * self.W if self.with_maps else 1, np.uint32)

    def __call__(self, jobs, engine, bitmaps=True):
        q = np.zeros(len(jobs), Q_DT); q["job"] = jobs; q["group"] = -1; q["podset"] = -1; q["nodeset"] = -1
        ans = np.zeros(len(jobs) * 6, np.int32)
        pm = abi.KaiSubsetParams(abi.SUBSET_VERSION, abi.SUBSET_ENGINE_PATH if engine else 0)
        for _ in range(2):  # (the capacity protocol: a call that needs more room says how much; the warm-up call of every M meets it)
            maps = bitmaps and self.with_maps
            t0 = time.perf_counter()
            rc = self.lib.kai_subset_nodes(self.h, C.byref(pm), q.ctypes.data_as(C.POINTER(abi.KaiSubsetQuery)), len(q), None, 0, ans.ctypes.data_as(C.POINTER(abi.KaiSubsetAnswer)),
                                           self.sets.ctypes.data_as(C.POINTER(abi.KaiNodeSet)), self.cap, C.byref(self.n),
                                           self.maps.ctypes.data_as(C.POINTER(C.c_uint32)) if maps else None, C.byref(self.res))
            ms = (time.perf_counter() - t0) * 1e3
            if rc != -4: break
            self.room(int(self.n.value))
        assert rc == 0, (rc, self.lib.kai_last_error(self.h))
        n = int(self.n.value)
        return ms, ans.copy(), self.sets[: 4 * n].copy(), (self.maps[: n * self.W].copy() if maps else None), self.res.path


def split_child(keys, scale):
    """one warm-up and one call per configuration, session and M under KAI_SUBSET_PROF (set by the parent): the library prints the split"""
    for key in keys:
        snap, cfg, _, jobs = load(key, scale)
        if not len(jobs): continue
        with pkg.KaiCore(cfg) as core:
            ssn = core.open_session(snap)
            call = Caller(core, snap)
            for name in ("fresh", "after_allocate"):
                if name == "after_allocate": ssn.execute("allocate")
                for m in COUNTS:
                    call(np.resize(jobs, m), False)
                    sys.stderr.write(f"kai subset nodes session {key} {name} {m}\n"); sys.stderr.flush()
                    call(np.resize(jobs, m), False)
            ssn.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--engine-cap-s", type=float, default=20.0)
    ap.add_argument("--configs", default="3,4m")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_nodes_timing_c4.json"))
    ap.add_argument("--split-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    keys = [k for k in a.configs.split(",") if k]
    if a.split_child: return split_child(keys, a.scale)
    out = dict(scale=a.scale, runs=a.runs, engine_cap_s=a.engine_cap_s, configs={})
    for key in keys:
        snap, cfg, desc, jobs = load(key, a.scale)
        c = dict(config=desc, nodes=snap.n_nodes, pods=snap.n_pods, jobs=snap.n_jobs, domains=int(len(snap.arrays["domain_parent"])) if "domain_parent" in snap.arrays else 0,
                 topology_gangs=int(len(jobs)), sessions={})
        out["configs"][key] = c
        if not len(jobs): continue
        with pkg.KaiCore(cfg) as core:
            ssn = core.open_session(snap)
            call = Caller(core, snap)
            for name in ("fresh", "after_allocate"):
                if name == "after_allocate": ssn.execute("allocate")
                s = {}; ms_per_query = None
                for m in COUNTS:
                    qj = np.resize(jobs, m)
                    call(qj, False)  # warm-up: the handle's scratch and staging grow here, the kernels' code objects load
                    runs = [call(qj, False) for _ in range(a.runs)]
                    _, ans, sets, maps, path = runs[-1]
                    r = dict(distinct_gangs=int(min(m, len(jobs))), sets=int(len(sets) // 4), bitmaps=maps is not None, path=PATHS[path], wide_ms=[round(x[0], 3) for x in runs], wide_median_ms=round(statistics.median(x[0] for x in runs), 3))
                    nb = [call(qj, False, bitmaps=False)[0] for _ in range(a.runs)]
                    r["wide_no_bitmaps_median_ms"] = round(statistics.median(nb), 3)
                    est_s = None if ms_per_query is None else ms_per_query * m / 1e3
                    if est_s is not None and est_s > a.engine_cap_s:
                        r["engine"] = "skipped"; r["engine_estimate_s"] = round(est_s, 1)
                    else:
                        ems, eans, esets, emaps, epath = call(qj, True)
                        assert PATHS[epath] == "engine" and np.array_equal(ans, eans) and np.array_equal(sets, esets) and (maps is None or np.array_equal(maps, emaps)), f"{key} {name} M {m}: the two paths differ"
                        r["engine_ms"] = round(ems, 3); r["engine_ms_per_query"] = round(ems / m, 3); r["engine_over_wide"] = round(ems / r["wide_median_ms"], 1)
                        ms_per_query = ems / m
                    if m <= 64:
                        t0 = time.perf_counter()
                        for j in qj: call(np.array([j], np.int32), False)
                        r["one_query_calls_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                    s[str(m)] = r
                c["sessions"][name] = s
            ssn.close()
    # the per-launch split, in a process of its own
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child", "--scale", str(a.scale), "--configs", a.configs], env=dict(os.environ, KAI_SUBSET_PROF="1"),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    where = None
    for ln in r.stderr.splitlines():
        m = re.match(r"kai subset nodes session (\w+) (\w+) (\d+)", ln)
        if m: where = m.groups(); continue
        m = re.match(r"kai subset nodes: path (\d+) sets (\d+) \|(.*) ms$", ln)
        if m and where:
            toks = m.group(3).split()
            rec = out["configs"][where[0]]["sessions"][where[1]][where[2]]
            rec["launch_split_ms"] = {toks[i]: float(toks[i + 1]) for i in range(0, len(toks), 2)}
            rec["launch_split_sum_ms"] = round(sum(float(toks[i + 1]) for i in range(0, len(toks), 2)), 4)
            where = None
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
