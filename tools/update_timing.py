"""kai_session_update against kai_session_open at config 5 (65 536 nodes x 1.06 M pods) on the MI355X.

  1. open S and run allocate;
  2. the delta the next cycle carries (abi.next_cycle_delta): the placed pods Running at their nodes, the pipelined ones Pending, 1 % of the running
     pods Succeeded — and two smaller deltas, its first 10 % and 1 % of pods;
  3. wall time of open(S') against update(delta) in the steady state: ONE session takes the delta and its inverse in turn, K times each, so every timed
     update after the first pays what a scheduler pays cycle after cycle (the first update of a session, with its one-time uploads, is reported apart);
     the library's host clocks (KAI_PROF) split each update into staging + gather + checks, host bookkeeping and device work;
  4. the allocate that follows is hash-equal either way.

--open-ab LIB: also time kai_session_open of S with another build of the library (e.g. the parent commit's) in alternating child processes
(--ab-procs of each, 2 by default; the medians of every process are reported beside the overall ones).
Prints one JSON line; --out writes it to a file too.  Usage: python tools/update_timing.py [--scale 1.0] [--runs 7] [--open-ab LIB [--ab-procs 2]] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as _entry  # noqa: E402

pkg = _entry._load_pkg()
PROF = re.compile(r"kai update: (\d+) pods (\d+) nodes(?: \d+ queue rows \d+ job rows)? \| stage \+ gather \+ checks ([\d.]+), host bookkeeping ([\d.]+), device \(scatter, classes, re-derivation\) ([\d.]+) \| total ([\d.]+) ms")


def ops_hash(ops):
    import hashlib
    h = hashlib.sha256()
    for o in ops:
        h.update(np.array([int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"])], np.int64).tobytes())
    return h.hexdigest()


class StderrCapture:
    """The library's stderr lines (KAI_PROF) while a call runs: fd 2 redirected into a temporary file."""
    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile(mode="w+b"); self.saved = os.dup(2); os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.f.seek(0); self.text = self.f.read().decode(errors="replace"); self.f.close()


def inverse(snap, d):
    """The delta that takes S' back to S."""
    pods = list(d["pods"])
    return dict(pods=pods, status=[int(snap.pod_status[p]) for p in pods], node=[int(snap.pod_node[p]) for p in pods])


def time_updates(core, snap, d, runs):
    """Steady state on one session: d, inverse, d, ... — wall ms and the library's split of every update."""
    lib, h = core.lib, core.handle
    dfw, kf = pkg.core.delta_struct(d["pods"], d["status"], d["node"])
    inv = inverse(snap, d)
    dbw, kb = pkg.core.delta_struct(inv["pods"], inv["status"], inv["node"])
    walls, split = [], []
    for i in range(2 * runs):
        ds = dfw if i % 2 == 0 else dbw
        with StderrCapture() as cap:
            t0 = time.perf_counter(); rc = lib.kai_session_update(h, C.byref(ds)); t1 = time.perf_counter()
        assert rc == 0, lib.kai_last_error(h)
        walls.append((t1 - t0) * 1e3)
        m = PROF.search(cap.text)
        if m:
            split.append([float(m.group(k)) for k in (3, 4, 5)])
    return walls, split


def open_child(lib_path, scale, runs):
    code = f"""
import ctypes as C, json, sys, time
sys.path.insert(0, {ROOT!r})
import __graft_entry__ as e
pkg = e._load_pkg()
lib = C.CDLL({lib_path!r})
snap, cfg, _ = pkg.synth.config(4, {scale})
st = snap.as_struct()
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
ts = []
for _ in range({runs} + 1):
    t0 = time.perf_counter(); rc = lib.kai_session_open(h, C.byref(st)); t1 = time.perf_counter()
    assert rc == 0
    ts.append((t1 - t0) * 1e3)
lib.kai_core_destroy(h)
print(json.dumps(ts[1:]))
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-1500:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--open-ab")
    ap.add_argument("--ab-procs", type=int, default=2)  # child processes per library
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["KAI_PROF"] = "1"
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    rng = np.random.default_rng(7)
    res = {"config": desc, "pods": snap.n_pods, "nodes": snap.n_nodes, "runs": a.runs, "deltas": []}
    equal = True
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        ops = core.open_session(snap).execute("allocate")
        full = pkg.abi.next_cycle_delta(snap, ops, rng)
        st_s = snap.as_struct()
        for frac in (1.0, 0.1, 0.01):
            k = max(1, int(len(full["pods"]) * frac))
            d = {key: v[:k] for key, v in full.items()}
            s2 = pkg.abi.apply_delta(snap, **d)
            st2 = s2.as_struct()
            t_open = []
            for _ in range(a.runs):
                with StderrCapture():
                    t0 = time.perf_counter(); rc = lib.kai_session_open(h, C.byref(st2)); t1 = time.perf_counter()
                assert rc == 0, lib.kai_last_error(h)
                t_open.append((t1 - t0) * 1e3)
            h_open = ops_hash(pkg.core.Session(core, s2).execute("allocate"))
            # one session on S: its first update (one-time uploads), then the steady state
            with StderrCapture():
                assert lib.kai_session_open(h, C.byref(st_s)) == 0
            dfirst, keep = pkg.core.delta_struct(d["pods"], d["status"], d["node"])
            with StderrCapture() as cap:
                t0 = time.perf_counter(); rc = lib.kai_session_update(h, C.byref(dfirst)); t1 = time.perf_counter()
            assert rc == 0, lib.kai_last_error(h)
            first = (t1 - t0) * 1e3
            back, kb = pkg.core.delta_struct(**inverse(snap, d))
            with StderrCapture():
                assert lib.kai_session_update(h, C.byref(back)) == 0
            walls, split = time_updates(core, snap, d, a.runs)  # ends on S (an even number of updates)
            with StderrCapture():
                assert lib.kai_session_update(h, C.byref(dfirst)) == 0
            h_upd = ops_hash(pkg.core.Session(core, s2).execute("allocate"))
            fw = walls[0::2]; sp = split[0::2]
            row = {"delta_pods": k, "open_ms_median": statistics.median(t_open), "update_ms_median": statistics.median(fw), "update_ms_first_of_session": first,
                   "update_ms_all": [round(x, 3) for x in walls], "allocate_hash_equal": h_open == h_upd}
            if sp:
                row["update_split_ms_median"] = {"stage_gather_checks": statistics.median(x[0] for x in sp), "host_bookkeeping": statistics.median(x[1] for x in sp),
                                                 "device": statistics.median(x[2] for x in sp)}
            equal = equal and h_open == h_upd
            res["deltas"].append(row)
    if a.open_ab:
        this_lib = os.path.join(ROOT, "kai-scheduler_amd", "csrc", "libkai_core.so")
        ta, tb, ma, mb = [], [], [], []
        for _ in range(a.ab_procs):  # alternating child processes: A B A B ...
            xa = open_child(a.open_ab, a.scale, a.runs); xb = open_child(this_lib, a.scale, a.runs)
            ta += xa; tb += xb; ma.append(round(statistics.median(xa), 3)); mb.append(round(statistics.median(xb), 3))
        res["open_ab"] = {"other_lib_ms_median": statistics.median(ta), "this_lib_ms_median": statistics.median(tb), "other_lib_ms": [round(x, 3) for x in ta],
                          "this_lib_ms": [round(x, 3) for x in tb], "other_lib_process_medians": ma, "this_lib_process_medians": mb}
    res["allocate_hash_equal"] = equal
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
