"""kai_job_order at config 5's full size on the MI355X.

Three sessions of one handle: config 5 as opened ("fresh"), the same with depth = 8 ("depth8"), and config 5 after one allocate ("after_allocate").  On each:
 - the chip-wide path: median over --runs calls through ctypes (a host clock around a call that ends in a stream synchronise), after one warm-up call that grows the
   handle's scratch;
 - the engine path (KAI_JOB_ORDER_ENGINE_PATH) on the same session.  It walks one heap pop after the other on one lane: the depth-8 session runs first, and where its
   time per pop says that a session would take more than --engine-cap-s seconds, that session's engine run is skipped and the estimate is written down instead;
 - the two paths must return the same order and positions;
 - the per-launch split of the chip-wide path: a child process of its own with KAI_JOB_ORDER_PROF=1 (the library waits for every launch between two events and prints the
   milliseconds per kernel), so that the end-to-end figures above are taken without it.
No bar is set: every figure is written down, beside the full plan of an allocate cycle (profiles/r06y_C5_kernels_per_round.txt) for comparison.

Prints one JSON line and writes it to --out (default profiles/job_order_timing_c5.json).
Usage: python tools/job_order_timing.py [--scale 1.0] [--runs 7] [--engine-cap-s 60] [--out FILE]"""
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
PATHS = {abi.JOB_ORDER_PATH_NONE: "none", abi.JOB_ORDER_PATH_WIDE: "wide", abi.JOB_ORDER_PATH_ENGINE: "engine"}
SESSIONS = (("depth8", False, 8), ("fresh", False, -1), ("after_allocate", True, -1))  # (name, one allocate first, depth)


class Caller:
    def __init__(self, core, J):
        self.lib, self.h, self.J = core.lib, core.handle, J
        self.order, self.pos, self.qpos = np.zeros(max(J, 1), np.int32), np.zeros(max(J, 1), np.int32), np.zeros(max(J, 1), np.int32)
        self.n, self.res = C.c_int32(0), abi.KaiJobOrderResult()

    def __call__(self, depth, engine):
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        pm = abi.KaiJobOrderParams(abi.JOB_ORDER_VERSION, abi.JOB_ORDER_ENGINE_PATH if engine else 0, depth, 0)
        t0 = time.perf_counter()
        rc = self.lib.kai_job_order(self.h, C.byref(pm), ip(self.order), self.J, C.byref(self.n), ip(self.pos), ip(self.qpos), C.byref(self.res))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, self.lib.kai_last_error(self.h))
        return ms, self.order[: self.n.value].copy(), self.pos.copy(), self.qpos.copy(), self.res.path


def split_child(scale):
    """one warm-up and one call per session under KAI_JOB_ORDER_PROF (set by the parent): the library prints the split"""
    snap, cfg, _ = pkg.synth.config(4, scale)
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        call = Caller(core, snap.n_jobs)
        done_allocate = False
        for name, allocate, depth in SESSIONS:
            if allocate and not done_allocate: ssn.execute("allocate"); done_allocate = True
            call(depth, False)
            sys.stderr.write(f"kai job order session {name}\n"); sys.stderr.flush()
            call(depth, False)
        ssn.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--engine-cap-s", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "job_order_timing_c5.json"))
    ap.add_argument("--split-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.split_child: return split_child(a.scale)
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    out = dict(config=desc, scale=a.scale, nodes=snap.n_nodes, pods=snap.n_pods, jobs=snap.n_jobs, queues=snap.n_queues, runs=a.runs, engine_cap_s=a.engine_cap_s, sessions={})
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        call = Caller(core, snap.n_jobs)
        us_per_pop = None; done_allocate = False
        for name, allocate, depth in SESSIONS:
            if allocate and not done_allocate: ssn.execute("allocate"); done_allocate = True
            call(depth, False)  # warm-up: the handle's scratch and staging grow here, the kernels' code objects load
            runs = [call(depth, False) for _ in range(a.runs)]
            _, order, pos, qpos, path = runs[-1]
            s = dict(depth=depth, ordered=int(len(order)), path=PATHS[path], wide_ms=[round(r[0], 3) for r in runs], wide_median_ms=round(statistics.median(r[0] for r in runs), 3))
            est_s = None if us_per_pop is None else us_per_pop * len(order) / 1e6
            if est_s is not None and est_s > a.engine_cap_s:
                s["engine"] = "skipped"; s["engine_estimate_s"] = round(est_s, 1)
            else:
                eruns = [call(depth, True) for _ in range(2 if us_per_pop is None else 1)]
                ems, eorder, epos, eqpos, epath = eruns[-1]
                assert PATHS[epath] == "engine" and np.array_equal(order, eorder) and np.array_equal(pos, epos) and np.array_equal(qpos, eqpos), f"{name}: the two paths differ"
                s["engine_ms"] = [round(r[0], 3) for r in eruns]; s["engine_last_ms"] = round(ems, 3); s["engine_us_per_pop"] = round(ems * 1e3 / max(len(order), 1), 3)
                s["engine_over_wide"] = round(ems / s["wide_median_ms"], 1)
                if us_per_pop is None: us_per_pop = ems * 1e3 / max(len(order), 1)
            out["sessions"][name] = s
        ssn.close()
    # the per-launch split, in a process of its own
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--split-child", "--scale", str(a.scale)], env=dict(os.environ, KAI_JOB_ORDER_PROF="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name = None
    for ln in r.stderr.splitlines():
        m = re.match(r"kai job order session (\w+)", ln)
        if m: name = m.group(1); continue
        m = re.match(r"kai job order: path (\d+) ordered (\d+) \|(.*) ms$", ln)
        if m and name:
            toks = m.group(3).split()
            out["sessions"][name]["launch_split_ms"] = {toks[i]: float(toks[i + 1]) for i in range(0, len(toks), 2)}
            out["sessions"][name]["launch_split_sum_ms"] = round(sum(float(toks[i + 1]) for i in range(0, len(toks), 2)), 4)
            name = None
    out["full_plan_of_an_allocate_cycle_ms"] = 0.53  # profiles/r06y_C5_kernels_per_round.txt: leaf 0.10, rank 0.21, gather 0.06, scans 0.07 + 0.07, setup / emit 0.03
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
