"""kai_ops_apply at config 5's full size on the MI355X: the device's own allocate operations (about 150 k) taken back into a freshly reset session.

 - the chip-wide path: median over --runs resets (each run: kai_session_reset, then ONE kai_ops_apply through ctypes with the array built beforehand; the call ends in
   a stream synchronise), after one warm-up call that grows the handle's scratch;
 - the engine walk on the same batch (KAI_APPLY_ENGINE_PATH): ONE run — the baseline, made of the engine's Statement code as it was before this entry point existed;
 - for context, kai_session_update with the equivalent pod delta (the placed pods as Binding on their nodes), which re-derives the whole session.
After every apply the pod states must equal the ones the allocate action itself left.  No ratio is fixed in advance: both numbers are written down.

One process.  Prints one JSON line and writes it to --out (default profiles/ops_apply_timing_c5.json).  Usage: python tools/ops_apply_timing.py [--scale 1.0] [--runs 5] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ops_apply_timing_c5.json"))
    a = ap.parse_args()
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    out = dict(config=desc, scale=a.scale, nodes=snap.n_nodes, pods=snap.n_pods, runs=a.runs)
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        ssn = core.open_session(snap)
        ops = ssn.execute("allocate")
        st_ref, nd_ref = ssn.pod_states()
        out["operations"] = int(len(ops)); out["statements"] = int(len(np.unique(ops["stmt"])))
        ptr = ops.ctypes.data_as(C.POINTER(abi.KaiOp))
        res = abi.KaiApplyResult()

        def apply(flags):
            ssn.reset()
            t0 = time.perf_counter()
            rc = lib.kai_ops_apply(h, ptr, len(ops), flags, C.byref(res))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, lib.kai_last_error(h))
            st, nd = ssn.pod_states()
            assert (st == st_ref).all() and (nd == nd_ref).all(), "the applied state differs from the action's own"
            return ms, res.path

        apply(0)  # warm-up: the handle's scratch and staging grow here
        wide = [apply(0) for _ in range(a.runs)]
        assert all(p == abi.APPLY_PATH_WIDE for _, p in wide), "the batch did not take the chip-wide path"
        out["wide_ms"] = [round(m, 3) for m, _ in wide]; out["wide_median_ms"] = round(statistics.median(m for m, _ in wide), 3)
        ms, path = apply(abi.APPLY_ENGINE_PATH)
        assert path == abi.APPLY_PATH_ENGINE
        out["engine_ms"] = round(ms, 3)
        # context: the same pods through kai_session_update (Binding on their nodes): a re-derivation of the whole session
        ssn.reset()
        pods = np.ascontiguousarray(ops["pod"], np.int32)
        d, keep = pkg.core.delta_struct(pods, np.full(len(pods), abi.POD_STATUS["Binding"], np.int32), np.ascontiguousarray(ops["node"], np.int32))
        t0 = time.perf_counter()
        rc = lib.kai_session_update(h, C.byref(d))
        out["session_update_ms"] = round((time.perf_counter() - t0) * 1e3, 3); out["session_update_status"] = int(rc)
        ssn.close()
    out["wide_over_engine"] = round(out["wide_median_ms"] / out["engine_ms"], 5) if out["engine_ms"] else None
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
