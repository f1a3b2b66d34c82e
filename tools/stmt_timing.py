"""kai_stmt_* at config 5's full size on the MI355X: the device's own allocate operations (about 150 k) as an open Statement.

For n = 1, 1 024 and all operations, each call timed by a host clock around it (every call ends in its own stream synchronise):
 - apply / rollback: the Statement holds the first (all - n) operations; kai_stmt_apply of the last n, then kai_stmt_rollback to the checkpoint in front of them;
 - commit: a Statement whose log is the first n operations and nothing else; kai_stmt_commit with the operations handed back;
on the chip-wide path and on the engine walk (KAI_APPLY_ENGINE_PATH for every call of the run, the prefix included), each the median over --runs runs after a warm-up
run that grows the handle's buffers.  Against it the only undo a caller had before: kai_session_reset followed by kai_ops_apply of the surviving prefix (the same first
(all - n) operations, chip-wide), with a device synchronise behind it, median over --runs.
After every rollback the pod states must equal those of the prefix alone, after every commit those of kai_ops_apply of the same operations.  No figure is fixed in advance.

One process.  Prints one JSON line and writes it to --out (default profiles/stmt_timing_c5.json).  Usage: python tools/stmt_timing.py [--scale 1.0] [--runs 5] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stmt_timing_c5.json"))
    a = ap.parse_args()
    snap, cfg, desc = pkg.synth.config(4, a.scale)
    out = dict(config=desc, scale=a.scale, nodes=snap.n_nodes, pods=snap.n_pods, runs=a.runs)
    with pkg.KaiCore(cfg) as core:
        lib, h = core.lib, core.handle
        hip = pkg.core._hip_runtime()
        ssn = core.open_session(snap)
        ops = ssn.execute("allocate")
        st_ref, nd_ref = ssn.pod_states()
        total = int(len(ops)); out["operations"] = total
        ptr = lambda lo: C.cast(C.c_void_p(ops.ctypes.data + lo * ops.itemsize), C.POINTER(abi.KaiOp))
        back = np.zeros(total, ops.dtype); res = abi.KaiStmtResult(); ares = abi.KaiApplyResult(); got = C.c_int64(0)

        def timed(fn, *args):
            t0 = time.perf_counter()
            rc = fn(h, *args)
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, lib.kai_last_error(h))
            return ms

        def prefix_state(m):
            """pod states of kai_ops_apply of the first m operations: (committed, as an open Statement leaves them)"""
            ssn.reset()
            if m: assert lib.kai_ops_apply(h, ptr(0), m, 0, C.byref(ares)) == 0
            st, nd = ssn.pod_states()
            un = st.copy(); un[un == abi.POD_STATUS["Binding"]] = abi.POD_STATUS["Allocated"]  # an open Statement leaves Allocated
            return st.copy(), un, nd.copy()

        def one(n, flags):
            m = total - n
            ssn.reset()
            assert lib.kai_stmt_begin(h, abi.STMT_VERSION) == 0
            if m: timed(lib.kai_stmt_apply, ptr(0), m, flags, C.byref(res))
            t_apply = timed(lib.kai_stmt_apply, ptr(m), n, flags, C.byref(res)); p_apply = res.path
            t_back = timed(lib.kai_stmt_rollback, m, flags, C.byref(res)); p_back = res.path
            st, nd = ssn.pod_states()
            assert (st == want[m][1]).all() and (nd == want[m][2]).all(), "the rolled-back state differs from the prefix's"
            assert lib.kai_stmt_discard(h, flags, C.byref(res)) == 0
            # the commit of a log of n records
            assert lib.kai_stmt_begin(h, abi.STMT_VERSION) == 0
            timed(lib.kai_stmt_apply, ptr(0), n, flags, C.byref(res))
            t_commit = timed(lib.kai_stmt_commit, back.ctypes.data_as(C.POINTER(abi.KaiOp)), total, C.byref(got), C.byref(res)); p_commit = res.path
            st, nd = ssn.pod_states()
            assert got.value == n and (st == want[n][0]).all() and (nd == want[n][2]).all(), "the committed state differs from kai_ops_apply's"
            assert (back["pod"][:n] == ops["pod"][:n]).all() and (back["node"][:n] == ops["node"][:n]).all() and (back["kind"][:n] == ops["kind"][:n]).all()
            return (t_apply, t_back, t_commit), (p_apply, p_back, p_commit)

        def reset_and_reapply(n):
            m = total - n
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            assert lib.kai_session_reset(h) == 0
            if m: assert lib.kai_ops_apply(h, ptr(0), m, 0, C.byref(ares)) == 0
            hip.hipDeviceSynchronize()
            return (time.perf_counter() - t0) * 1e3

        sizes = sorted({min(1, total), min(1024, total), total})
        want = {m: prefix_state(m) for m in sorted({total - n for n in sizes} | set(sizes))}
        one(total, 0); one(sizes[0], 0); one(sizes[0], abi.APPLY_ENGINE_PATH)  # warm-up: the handle's buffers and the engine's scratch grow here
        for n in sizes:
            key = "all" if n == total else str(n)
            for name, flags, path in (("wide", 0, abi.APPLY_PATH_WIDE), ("engine", abi.APPLY_ENGINE_PATH, abi.APPLY_PATH_ENGINE)):
                runs = [one(n, flags) for _ in range(a.runs)]
                assert all(p == (path,) * 3 for _, p in runs), f"a call did not take the {name} path"
                for i, what in enumerate(("apply", "rollback", "commit")):
                    out[f"{name}_{what}_{key}_ms"] = [round(t[i], 3) for t, _ in runs]; out[f"{name}_{what}_{key}_median_ms"] = round(statistics.median(t[i] for t, _ in runs), 3)
            base = [reset_and_reapply(n) for _ in range(a.runs)]
            out[f"reset_reapply_{key}_ms"] = [round(x, 3) for x in base]; out[f"reset_reapply_{key}_median_ms"] = round(statistics.median(base), 3)
        ssn.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
