"""Spread placement on the GPU (gpu_strategy = SPREAD) at config 5 (65 536 nodes x 1.06 M pods) and config 2 (1 000 nodes x 10 k pods) on the MI355X,
through the C ABI: the allocate action on the sets (the spread instantiations of k_fill_levels / k_fill_counts) against the general kernel (KAI_FILL_GENERAL=1).

A cycle is kai_session_reset + allocate on the HBM-resident snapshot, `--warmup` cycles untimed.  Every run is a fresh child process (the environment
switches are read by the library; a process keeps its clocks, caches and LDS ceilings to itself); the two kinds of run alternate, `--reps` times each.
One JSON line per run: ms per cycle (median and all), the fill's ms, the fill kernel, rounds, decisions, SHA-256 of the operations.  The tool fails if
two runs of one config end with different operations.

--other-lib LIB: a third kind of run, with another build of the library (e.g. the parent commit's), alternating with the two.
Usage: python tools/spread_timing.py [--configs 5,2] [--scale 1.0] [--steps 5] [--warmup 2] [--reps 1] [--other-lib LIB] [--prof] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import hashlib, json, statistics, sys, time
import numpy as np
sys.path.insert(0, {root!r})
import __graft_entry__ as e
pkg = e._load_pkg()
if {lib!r}: pkg.load_library({lib!r})
snap, cfg, desc = pkg.synth.config({idx}, {scale})
cfg.gpu_strategy = pkg.abi.SPREAD
ts = []
with pkg.KaiCore(cfg) as core:
    ssn = core.open_session(snap)
    for i in range({warmup} + {steps}):
        t0 = time.perf_counter(); ssn.reset(); ops = ssn.execute("allocate"); t1 = time.perf_counter()
        if i >= {warmup}: ts.append((t1 - t0) * 1e3)
    st = ssn.stats()
    h = hashlib.sha256(np.stack([ops[k].astype(np.int64) for k in ("kind", "pod", "node", "job")], axis=1).tobytes()).hexdigest()
    ssn.close()
r1, r7 = int(st.reserved[1]), int(st.reserved[7])
batch = int(st.reserved[4]) > 0
kernel = "sequential engine" if not batch else "k_fill_levels" if (r1 >> 60) & 1 else "k_fill_counts" if (r1 >> 61) & 1 else "k_fill_buckets" if (r1 >> 62) & 1 else "k_fill"
print(json.dumps(dict(config=desc, strategy="spread", run={label!r}, ms_per_cycle=statistics.median(ts), ms_all=[round(x, 3) for x in ts], fill_ms=((r7 >> 21) & 0x1fffff) / 1e3 if batch else None,
                      plan_ms=(r7 >> 42) / 1e3 if batch else None, apply_ms=(r7 & 0x1fffff) / 1e3 if batch else None, fill_kernel=kernel, rounds=int(st.reserved[4]), decisions=int(st.decisions),
                      committed=int(st.jobs_committed), operations=len(ops), sha256=h)))
"""


def run_child(idx, scale, steps, warmup, label, general, lib, prof=False):
    env = dict(os.environ)
    env.pop("KAI_FILL_GENERAL", None); env.pop("KAI_PROF", None)
    if prof:
        env["KAI_PROF"] = "1"  # the library's own line per action on stderr: the fill's cycle clocks and command count (kai_action.hpp action_stats)
    if general:
        env["KAI_FILL_GENERAL"] = "1"
    code = CHILD.format(root=ROOT, lib=lib or "", idx=idx, scale=scale, steps=steps, warmup=warmup, label=label)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{label}: exit {r.returncode}\n{r.stderr[-1500:]}")
    row = json.loads(r.stdout.strip().splitlines()[-1])
    if prof:
        row["prof"] = ([ln for ln in r.stderr.splitlines() if ln.startswith("kai batch")] or [""])[-1]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="5,2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--other-lib")
    ap.add_argument("--prof", action="store_true", help="KAI_PROF=1 in the children: each row carries the library's last 'kai batch' line (cycle clocks of the fill's wavefronts, commands)")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines, equal = [], True
    for cfg_no in [int(x) for x in a.configs.split(",")]:
        kinds = ([("other build", False, a.other_lib)] if a.other_lib else []) + [("general kernel (KAI_FILL_GENERAL=1)", True, None), ("sets", False, None)]
        hashes = set()
        for _ in range(a.reps):
            for label, general, lib in kinds:  # alternating: a drift of the machine hits every kind alike
                row = run_child(cfg_no - 1, a.scale, a.steps, a.warmup, label, general, lib, a.prof)
                hashes.add(row["sha256"])
                lines.append(row)
                print(json.dumps(row), flush=True)
        if len(hashes) != 1:
            equal = False
            print(f"config {cfg_no}: the runs ended with different operations: {sorted(hashes)}", file=sys.stderr)
        for label, _, _ in kinds:
            ms = [r["ms_per_cycle"] for r in lines if r["run"] == label and r["config"].startswith(f"C{cfg_no} ")]
            if ms:
                print(json.dumps({"config": cfg_no, "run": label, "processes": len(ms), "ms_per_cycle_median": statistics.median(ms), "min": min(ms), "max": max(ms)}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
