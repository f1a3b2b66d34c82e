"""kai_stmt_* (an open Statement on the handle: apply, checkpoint, rollback, discard, commit) without a GPU.

 - the exports, the ABI struct, the header's text;
 - arguments and call order under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp): every host-decidable refusal is made
   before the first device call and leaves the device image as it was; the call order is enforced; a warm apply, rollback or commit allocates nothing; a checkpoint makes no
   device call;
 - the kernel bodies and the calls' control flow (kai_stmt.hpp) run with emulated lanes by tests/host_sim/stmt_sim.cpp on a session of the host simulation: the state behind
   every call against the oracle's Statement (tests/test_oracle_statement.py run_script) and against twins, on both paths, with workgroups of 256, 100 and 1 lanes.
   The composed walk (subset_nodes, ordered_nodes, apply, rollback, commit) runs there too, against the oracle's allocate.
The parity claim on the device is tests/test_gpu_stmt.py."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)
from test_gpu_parity import crowded
import test_ops_apply as OA
import test_oracle_statement as TOS
import test_oracle_topology_kat as KAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
S = abi.POD_STATUS
ALLOCATE, PIPELINE, EVICT = 0, 1, 2  # kai_op_kind
WIDE, ENGINE = abi.APPLY_PATH_WIDE, abi.APPLY_PATH_ENGINE
EP = abi.APPLY_ENGINE_PATH
BEGIN, APPLY, ROLLBACK, DISCARD, COMMIT, ACTION, OPS_APPLY, JOB_ORDER, SUBSET, BEST_NODES, ORDERED_NODES, WALK = range(12)  # kai_stsim_call.kind
CALL_DT = np.dtype([("kind", "<i4"), ("flags", "<u4"), ("lo", "<i8"), ("hi", "<i8")])
RET_DT = np.dtype([("status", "<i4"), ("path", "<i4"), ("first_bad", "<i8"), ("log_len", "<i8"), ("n_hidden", "<i8"), ("n_q", "<i8")])
N_TAIL = 6  # words of a hidden row behind the session's own: fast_ok, index_stale, open, ops_len, n_undo, non_allocate_commits (then the log)


def test_exports_and_struct_sizes():
    names = ["kai_stmt_begin", "kai_stmt_apply", "kai_stmt_checkpoint", "kai_stmt_rollback", "kai_stmt_discard", "kai_stmt_commit"]
    lib = T.pkg.load_library()
    for n in names:
        assert n in T.pkg.core.EXPORTS and hasattr(lib, n), n
    R = abi.KaiStmtResult
    assert C.sizeof(R) == 24 and [f[0] for f in R._fields_] == ["first_bad", "log_len", "path", "pad"]
    assert (R.first_bad.offset, R.log_len.offset, R.path.offset, R.pad.offset) == (0, 8, 16, 20) and abi.STMT_VERSION == 1
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    for text in ("#define KAI_STMT_VERSION 1u", "typedef struct kai_stmt_result { int64_t first_bad; int64_t log_len; int32_t path; int32_t pad; } kai_stmt_result;",
                 "int kai_stmt_begin(kai_core* core, uint32_t version);", "int kai_stmt_apply(kai_core* core, const kai_op* ops, int64_t n_ops, uint32_t flags, kai_stmt_result* result",
                 "int kai_stmt_checkpoint(kai_core* core, int64_t* cp_out);", "int kai_stmt_rollback(kai_core* core, int64_t cp, uint32_t flags, kai_stmt_result* result",
                 "int kai_stmt_discard(kai_core* core, uint32_t flags, kai_stmt_result* result", "int kai_stmt_commit(kai_core* core, kai_op* ops_out"):
        assert text in hdr, text
    assert hasattr(T.pkg.core.Session, "statement")
    for m in ("apply", "checkpoint", "rollback", "discard", "commit", "__enter__", "__exit__"):
        assert hasattr(T.pkg.core.Statement, m), m


# ---------------------------------------------------------------------------------------------- the host side under the host-only library
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
Op, Res = abi.KaiOp, abi.KaiStmtResult
lib.kai_stmt_begin.argtypes = [C.c_void_p, C.c_uint32]
lib.kai_stmt_apply.argtypes = [C.c_void_p, C.POINTER(Op), C.c_int64, C.c_uint32, C.POINTER(Res)]
lib.kai_stmt_checkpoint.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
lib.kai_stmt_rollback.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(Res)]
lib.kai_stmt_discard.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Res)]
lib.kai_stmt_commit.argtypes = [C.c_void_p, C.POINTER(Op), C.c_int64, C.POINTER(C.c_int64), C.POINTER(Res)]
lib.kai_ops_apply.argtypes = [C.c_void_p, C.POINTER(Op), C.c_int64, C.c_uint32, C.POINTER(abi.KaiApplyResult)]
lib.kai_action_execute.argtypes = [C.c_void_p, C.c_int, C.POINTER(Op), C.c_int64, C.POINTER(C.c_int64)]
lib.kai_stale_gang_eviction.argtypes = [C.c_void_p, C.POINTER(abi.KaiStaleParams), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(Op), C.c_int64, C.POINTER(C.c_int64), C.POINTER(abi.KaiStaleResult)]
snap, cfg, _ = pkg.synth.config(1, 0.3)
cfg = abi.copy_config(cfg); cfg.now_ns = 10**9
P, N, J = snap.n_pods, snap.n_nodes, snap.n_jobs
pending = [int(p) for p in np.nonzero(snap.arrays["pod_status"] == abi.POD_STATUS["Pending"])[0][:8]]
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def diff(a, b): return dict(allocations=b[1] - a[1], live_bytes=b[2] - a[2], launches=b[3] - a[3], h2d=b[4] - a[4], memsets=b[7] - a[7], pinned=b[8] - a[8])
def arr(ops): return (Op * max(len(ops), 1))(*[Op(77, k, p, nd, -5, st, pad) for k, p, nd, st, pad in ops])
def apply(h, ops, n=None, flags=0, null=False, res=True):
    r = Res(123, 45, 67, 89)
    rc = lib.kai_stmt_apply(h, None if null else arr(ops), len(ops) if n is None else n, flags, C.byref(r) if res else None)
    return [rc, r.first_bad, r.log_len, r.path]
def rollback(h, cp, flags=0):
    r = Res(123, 45, 67, 89); rc = lib.kai_stmt_rollback(h, cp, flags, C.byref(r)); return [rc, r.first_bad, r.log_len, r.path]
def discard(h, flags=0):
    r = Res(123, 45, 67, 89); rc = lib.kai_stmt_discard(h, flags, C.byref(r)); return [rc, r.first_bad, r.log_len, r.path]
def commit(h, cap, null=False):
    out = (Op * max(cap, 1))(); n = C.c_int64(-7); r = Res(123, 45, 67, 89)
    rc = lib.kai_stmt_commit(h, None if null else out, cap, C.byref(n), C.byref(r)); return [rc, n.value, r.log_len, r.path]
def checkpoint(h):
    cp = C.c_int64(-7); rc = lib.kai_stmt_checkpoint(h, C.byref(cp)); return [rc, cp.value]
def others(h):
    """the three calls an open Statement refuses"""
    n = C.c_int64(0); out = (Op * (2 * P + 64))(); ar = abi.KaiApplyResult()
    since = (C.c_int64 * J)(); sp = abi.KaiStaleParams(abi.STALE_VERSION, 0, 0); sr = abi.KaiStaleResult()
    return [lib.kai_action_execute(h, 0, out, 2 * P + 64, C.byref(n)), lib.kai_ops_apply(h, arr(good), len(good), 0, C.byref(ar)),
            lib.kai_stale_gang_eviction(h, C.byref(sp), since, None, out, P, C.byref(n), C.byref(sr))]
good = [(0, pending[0], 0, 0, 0), (0, pending[1], 1, 0, 0), (0, pending[2], N - 1, 1, 0), (0, pending[3], 2, 3, 0)]
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
res["before_open"] = [lib.kai_stmt_begin(h, 1), apply(h, good)[0], checkpoint(h)[0], rollback(h, 0)[0], discard(h)[0], commit(h, 8)[0]]
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = image()
res["without_begin"] = [apply(h, good), checkpoint(h), rollback(h, 0), discard(h), commit(h, 8)]
res["wrong_version"] = lib.kai_stmt_begin(h, 2)
res["image_unchanged_without_begin"] = image() == img0
res["begin"] = lib.kai_stmt_begin(h, 1); img1 = image()
res["begin_cost"] = diff(img0, img1)
res["double_begin"] = lib.kai_stmt_begin(h, 1)
bad = {}
bad["null_ops"] = apply(h, good, null=True)
bad["negative_count"] = apply(h, good, n=-1)
bad["unknown_flags"] = apply(h, good, flags=4)
bad["kind_3"] = apply(h, good[:2] + [(3, pending[4], 0, 0, 0)] + good[2:])
bad["pod_negative"] = apply(h, good[:2] + [(0, -1, 0, 0, 0)] + good[2:])
bad["pod_too_large"] = apply(h, good[:2] + [(0, P, 0, 0, 0)] + good[2:])
bad["node_negative"] = apply(h, good[:2] + [(0, pending[4], -1, 0, 0)] + good[2:])
bad["node_too_large"] = apply(h, good[:2] + [(2, pending[4], N, 0, 0)] + good[2:])
bad["pad"] = apply(h, good[:2] + [(0, pending[4], 0, 0, 9)] + good[2:])
bad["rollback_cp_negative"] = rollback(h, -1)
bad["rollback_cp_beyond"] = rollback(h, 1)
bad["rollback_flags"] = rollback(h, 0, flags=1)
bad["discard_flags"] = discard(h, flags=5)
bad["commit_negative_cap"] = commit(h, -1)
bad["commit_null_out"] = commit(h, 4, null=True)
bad["checkpoint_null"] = [lib.kai_stmt_checkpoint(h, None)]
res["bad"] = bad
res["too_long"] = apply(h, [(0, pending[0], 0, 0, 0)] * (2 * P + 33))
res["others_while_open"] = others(h)
res["empty"] = apply(h, []); res["rollback_to_len"] = rollback(h, 0); res["checkpoint0"] = checkpoint(h)
res["image_unchanged"] = image() == img1
# good calls: what each costs on the device (the kernels of the host-only library do nothing: the verdict that comes back is the one that was sent, "valid, every pod once")
res["apply1"] = apply(h, good); i1 = image()
res["stmt_decreases_is_fine"] = apply(h, [(0, pending[5], 0, 3, 0), (0, pending[6], 0, 1, 0)]); i2 = image()
res["checkpoint"] = checkpoint(h); res["checkpoint_image"] = image() == i2
res["warm_apply"] = diff(i1, i2)
res["rollback"] = rollback(h, 4); i3 = image()
res["apply3"] = apply(h, good[:1], res=False)[0]; i4 = image()
res["rollback2"] = rollback(h, 2); i5 = image()
res["warm_rollback"] = diff(i4, i5)
res["commit_small_cap"] = commit(h, 1); res["still_open"] = checkpoint(h)
i6 = image()
res["commit"] = commit(h, 8); i7 = image()
res["commit_cost"] = diff(i6, i7)
res["after_commit"] = [apply(h, good)[0], checkpoint(h)[0], lib.kai_stmt_begin(h, 1)]
res["apply_b"] = apply(h, good[2:]); i8 = image()
res["commit_b"] = commit(h, 8); i9 = image()
res["warm_commit"] = diff(i8, i9)
# what drops the Statement
res["begin_c"] = lib.kai_stmt_begin(h, 1); res["reset"] = lib.kai_session_reset(h); res["after_reset"] = [checkpoint(h)[0], lib.kai_stmt_begin(h, 1)]
assert lib.kai_session_open(h, C.byref(st)) == 0
res["after_reopen"] = [checkpoint(h)[0], lib.kai_stmt_begin(h, 1), discard(h)]
res["others_after_close"] = others(h)[1]
lib.kai_core_destroy(h)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["sharded"] = [lib.kai_stmt_begin(h2, 1), apply(h2, good)[0], commit(h2, 8)[0]]
lib.kai_core_destroy(h2)
snap3, cfg3, _ = pkg.synth.config(1, 0.2); pkg.synth.add_fractions(snap3, 7, frac=0.3)
h3 = C.c_void_p(); st3 = snap3.as_struct()
assert lib.kai_core_create(C.byref(cfg3), 1, None, C.byref(h3)) == 0 and lib.kai_session_open(h3, C.byref(st3)) == 0
img3 = image()
res["shared"] = [lib.kai_stmt_begin(h3, 1), apply(h3, [(0, 0, 0, 0, 0)])[0]]; res["shared_image_unchanged"] = image() == img3
lib.kai_core_destroy(h3)
print(json.dumps(res))
'''


def test_arguments_and_call_order(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["before_open"] == [-6] * 6, "KAI_ERR_STATE without an open session"
    assert [x[0] for x in out["without_begin"]] == [-6] * 5 and out["image_unchanged_without_begin"], "every call but begin needs an open Statement"
    assert out["wrong_version"] == -1
    assert out["begin"] == 0 and out["double_begin"] == -6
    assert out["begin_cost"]["launches"] == 0 and out["begin_cost"]["allocations"] == 1 and out["begin_cost"]["memsets"] == 2, out["begin_cost"]
    for k, v in out["bad"].items():
        assert v[0] == -1, (k, v)
    for k in ("kind_3", "pod_negative", "pod_too_large", "node_negative", "node_too_large", "pad"):
        assert out["bad"][k][1:] == [2, 0, 0], (k, out["bad"][k])
    assert out["too_long"][0] == -4, "KAI_ERR_CAPACITY: the log's room is 2 n_pods + 32"
    assert out["others_while_open"] == [-6, -6, -6], "actions, kai_ops_apply and stale-gang eviction are refused while a Statement is open"
    assert out["empty"] == [0, -1, 0, 0] and out["rollback_to_len"] == [0, -1, 0, 0] and out["checkpoint0"] == [0, 0]
    assert out["image_unchanged"], "a refused or empty call allocated or wrote device memory"
    assert out["apply1"] == [0, -1, 4, WIDE] and out["stmt_decreases_is_fine"] == [0, -1, 6, WIDE]
    assert out["checkpoint"] == [0, 6] and out["checkpoint_image"], "a checkpoint makes no device call"
    assert out["warm_apply"] == dict(allocations=0, live_bytes=0, launches=2, h2d=1, memsets=0, pinned=0), out["warm_apply"]
    assert out["rollback"] == [0, -1, 4, WIDE] and out["apply3"] == 0 and out["rollback2"] == [0, -1, 2, WIDE]
    assert out["warm_rollback"] == dict(allocations=0, live_bytes=0, launches=1, h2d=1, memsets=0, pinned=0), out["warm_rollback"]
    assert out["commit_small_cap"][:2] == [-4, 2] and out["still_open"] == [0, 2], "KAI_ERR_CAPACITY with *n_ops set leaves the Statement open"
    cc = out["commit_cost"]  # the first commit of a handle allocates the committed operations' device buffer
    assert out["commit"] == [0, 2, 0, WIDE] and (cc["allocations"], cc["launches"], cc["h2d"], cc["memsets"], cc["pinned"]) == (1, 1, 1, 0, 0), (out["commit"], cc)
    assert out["after_commit"] == [-6, -6, 0], "the commit closed the Statement"
    assert out["apply_b"] == [0, -1, 2, WIDE] and out["commit_b"] == [0, 2, 0, WIDE]
    assert out["warm_commit"] == dict(allocations=0, live_bytes=0, launches=1, h2d=1, memsets=0, pinned=0), out["warm_commit"]
    assert out["begin_c"] == 0 and out["reset"] == 0 and out["after_reset"] == [-6, 0], "kai_session_reset drops the Statement"
    assert out["after_reopen"] == [-6, 0, [0, -1, 0, 0]], "kai_session_open drops the Statement"
    assert out["others_after_close"] == 0
    assert out["sharded"] == [-5, -5, -5], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["shared"] == [-5, -5] and out["shared_image_unchanged"], "KAI_ERR_UNSUPPORTED in a session with shared-GPU requests, before the first device call"


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "stmt_sim.cpp")


def sim_lib():
    so = os.path.join(ROOT, "tests", "host_sim", "libstmtsim.so")
    deps = glob.glob(os.path.join(ROOT, "tests", "host_sim", "*.cpp")) + glob.glob(os.path.join(ROOT, "tests", "host_sim", "*.hpp")) + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_stsim_run.restype = C.c_int
    return lib


def _rows(buf, n, count, fields, inner):
    """a ctypes array of n x count structs of float64 fields -> per row a dict field -> [count, inner]"""
    raw = np.frombuffer(buf, dtype=np.float64).reshape(n, count, len(fields), -1)
    return [{f: raw[k, :, i, :inner].copy() for i, f in enumerate(fields)} for k in range(n)]


def sim_script(snap, cfg, ops, calls, lanes=256, batch=False, jobs=()):
    """calls: (kind, flags, lo, hi) tuples (tests/host_sim/stmt_sim.cpp kai_stsim_call) -> (per call a Result: status, path, first_bad, log_len, pod_status, pod_node, nodes,
    shares, hidden (the session's words, the tail, the log), q (the call's own output); the operations of the script's actions; the action statistics at the end)"""
    lib = sim_lib()
    s = snap.as_struct()
    P, Q, N, J = snap.n_pods, max(snap.n_queues, 1), max(snap.n_nodes, 1), snap.n_jobs
    ops = np.ascontiguousarray(ops, dtype=OA.OP_DT)
    ca = np.array([tuple(c) for c in calls], dtype=CALL_DT); K = len(ca)
    jb = np.ascontiguousarray(jobs, dtype=np.int32)
    ret = np.zeros(K, RET_DT)
    hs = 4 * P + 4 * snap.n_podsets + 8 * J + 8 + N_TAIL + 10 * (2 * P + 32)
    qs = 6 * (2 * P + 32) + 64 + 8 * J + 16 * len(jb)
    st, nd = np.zeros((K, P), np.int32), np.zeros((K, P), np.int32)
    sh = (abi.KaiQueueShare * (K * Q))(); ns = (abi.KaiNodeState * (K * N))()
    hid, qo = np.zeros((K, hs), np.int32), np.zeros((K, qs), np.int32)
    cap = max(64, 8 * P); out = (abi.KaiOp * cap)(); n_out = C.c_int64(0); stats = abi.KaiActionStats()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.kai_stsim_run(C.byref(cfg), C.byref(s), C.c_int(int(batch)), ops.ctypes.data_as(C.c_void_p), C.c_int64(len(ops)), ip(jb) if len(jb) else None, C.c_int64(len(jb)),
                           ca.ctypes.data_as(C.c_void_p), C.c_int(K), C.c_int(lanes), ret.ctypes.data_as(C.c_void_p), ip(st), ip(nd), sh, ns, ip(hid), C.c_int64(hs), ip(qo), C.c_int64(qs),
                           out, C.c_int64(cap), C.byref(n_out), C.byref(stats))
    assert rc == 0, f"kai_stsim_run rc={rc}"
    shares = _rows(sh, K, Q, [f[0] for f in abi.KaiQueueShare._fields_], 3)
    nodes = _rows(ns, K, N, [f[0] for f in abi.KaiNodeState._fields_], snap.n_res)
    res = [T.Result(status=int(ret[k]["status"]), path=int(ret[k]["path"]), first_bad=int(ret[k]["first_bad"]), log_len=int(ret[k]["log_len"]), pod_status=st[k], pod_node=nd[k],
                    nodes=nodes[k], shares=shares[k], hidden=hid[k, : ret[k]["n_hidden"]].copy(), q=qo[k, : ret[k]["n_q"]].copy()) for k in range(K)]
    return res, [(o.kind, o.pod, o.node, o.job) for o in out[: n_out.value]], stats


def same_readbacks(a, b, what=""):
    OA.same_state(a, b.pod_status, b.pod_node, b.nodes, b.shares, what)


def closed(r):
    """a result behind a commit, for the comparison with kai_ops_apply's: without the count of committed evictions / pipelines (EngineState::non_allocate_commits, the last
    word of a closed Statement's row: kai_ops_apply's chip-wide path leaves it to the host's fast_ok, which IS compared)"""
    assert r.log_len == 0
    h = r.hidden.copy(); h[-1] = 0
    return T.Result(pod_status=r.pod_status, pod_node=r.pod_node, nodes=r.nodes, shares=r.shares, hidden=h)


def same_all(a, b, what=""):
    same_readbacks(a, b, what)
    assert np.array_equal(a.hidden, b.hidden), f"{what}: the state no read-back shows, or the log, differs at words {np.nonzero(a.hidden != b.hidden)[0][:8].tolist() if len(a.hidden) == len(b.hidden) else (len(a.hidden), len(b.hidden))}"


# ---- (3) the oracle's Statement scripts
def script_shapes(sc):
    """the shapes of a script as lists of steps: ("apply", lo, hi) | ("rollback", cp) | ("discard",); each apply, rollback and discard is one device call"""
    n = len(sc); m = max(n // 2, 1)
    yield "cp-script-rollback", [("apply", 0, n), ("rollback", 0)]
    if n >= 2:
        yield "a-cp-b-rollback", [("apply", 0, m), ("apply", m, n), ("rollback", m)]
        yield "a-cp-b-rollback-c", [("apply", 0, m), ("apply", m, n), ("rollback", m), ("apply", m, n)]
        yield "a-cp-b-rollback-c-discard", [("apply", 0, m), ("apply", m, n), ("rollback", m), ("apply", m, n), ("discard",)]
    else:
        yield "script-discard", [("apply", 0, n), ("discard",)]


def _prefix_rows(sc, steps, k):
    """the rows of kai_oracle_statement_script for the state behind step k.  The log in front of step k is what the earlier steps left (earlier rollbacks collapsed: each
    is checked at its own step); an apply appends to it; a rollback is the oracle's own: the surviving prefix, a checkpoint, the rest, Rollback; a discard is its Discard"""
    log = []
    row = lambda i: (OA.TO_ORACLE[sc[i][0]], sc[i][1], sc[i][2], 1)
    for st in steps[:k]:
        if st[0] == "apply": log += list(range(st[1], st[2]))
        elif st[0] == "rollback": log = log[: st[1]]
        else: log = []
    st = steps[k]
    if st[0] == "apply": return [row(i) for i in log + list(range(st[1], st[2]))]
    if st[0] == "rollback": return [row(i) for i in log[: st[1]]] + [(TOS.CP, 0, 0, 0)] + [row(i) for i in log[st[1]:]] + [(TOS.ROLLBACK, 0, 0, 0)]
    return [row(i) for i in log] + [(5, 0, 0, 0)]


def oracle_state(snap, cfg, rows):
    """TOS.run_script; every operation of the rows must be legal for the oracle (a checkpoint's result is the log's length)"""
    r, st, nd, nodes = TOS.run_script(snap, cfg, rows)
    assert all(x for x, row in zip(r, rows) if row[0] != TOS.CP), r
    return r, st, nd, nodes


def run_steps(snap, cfg, sc, steps, lanes, engine):
    f = EP if engine else 0
    calls = [(BEGIN, 0, 0, 0)] + [(APPLY, f, st[1], st[2]) if st[0] == "apply" else (ROLLBACK, f, st[1], 0) if st[0] == "rollback" else (DISCARD, f, 0, 0) for st in steps]
    res, _, _ = sim_script(snap, cfg, OA.make_ops(sc), calls, lanes=lanes)
    assert all(r.status == 0 for r in res), [r.status for r in res]
    return res[1:]


SCRIPT_CASES = [(name, i, shape) for name, _, _, scripts in OA.script_sessions() for i, sc in enumerate(scripts) for shape, _ in script_shapes(sc)]


@pytest.fixture(scope="module")
def sessions():
    return {name: (snap, cfg, scripts) for name, snap, cfg, scripts in OA.script_sessions()}


@pytest.mark.parametrize("name,i,shape", SCRIPT_CASES, ids=[f"{n}-{i}-{s}" for n, i, s in SCRIPT_CASES])
def test_statement_scripts_against_the_oracle(sessions, name, i, shape):
    """checkpoint / operations / rollback / discard scripts: behind every device call pod status and node, node Idle / Releasing / Used as the oracle's Statement leaves them
    (Allocated against Allocated: nothing is committed); both paths and every workgroup size agree in everything, the hidden words and the log included"""
    snap, cfg, scripts = sessions[name]
    sc = scripts[i]; steps = dict(script_shapes(sc))[shape]
    named_twice = len({p for _, p, _ in sc}) < len(sc)
    first = None
    for engine in (False, True):
        for lanes in (256, 100, 1):
            res = run_steps(snap, cfg, sc, steps, lanes, engine)
            for k, r in enumerate(res):
                if engine: assert r.path in (ENGINE, 0), (k, r.path)
            if not engine and not named_twice:  # every pod once, from Pending / Running: every call of the script is the chip-wide path's
                assert all(r.path == WIDE for r in res), [r.path for r in res]
            if first is None:
                first = res
                for k in range(len(steps)):
                    r, st, nd, nodes = oracle_state(snap, cfg, _prefix_rows(sc, steps, k))
                    OA.same_state(res[k], np.array(st, np.int32), np.array(nd, np.int32), nodes, what=f"behind step {k} {steps[k]}")
            else:
                for k in range(len(steps)): same_all(res[k], first[k], f"engine {engine} lanes {lanes} step {k}")
    assert first[-1].log_len == (0 if steps[-1][0] == "discard" else steps[-1][1] if steps[-1][0] == "rollback" else steps[-1][2])


def config0_batches():
    snap, cfg = crowded(7)  # 13 nodes, 83 pods: 30 pending, 53 running
    cfg = abi.copy_config(cfg); cfg.plugins = 0  # the oracle's script runs a Statement on a session without plugins
    st, nd = snap.arrays["pod_status"], snap.arrays["pod_node"]
    pending = np.nonzero(st == S["Pending"])[0]; placed = np.nonzero((st == S["Running"]) & (nd >= 0))[0]
    assert len(pending) >= 26 and len(placed) >= 6
    N = snap.n_nodes
    once = [(ALLOCATE, int(p), int(i % N)) for i, p in enumerate(pending[:12])] + [(EVICT, int(p), int(nd[p])) for p in placed[:6]]
    again = [(EVICT, int(pending[0]), 0), (PIPELINE, int(placed[0]), int((nd[placed[0]] + 1) % N)), (ALLOCATE, int(pending[14]), 1)]  # two pods of `once` named again
    more = [(PIPELINE, int(p), int((3 * i + 1) % N)) for i, p in enumerate(pending[20:26])]
    return snap, cfg, once, again, more


@pytest.mark.parametrize("lanes", [256, 100, 1])
def test_the_paths_take_over_from_each_other(lanes):
    """a Statement that starts on the chip-wide path, goes on with a batch that names two of its pods again (the engine takes it), and is rolled back across the seam — and the
    reverse: a batch the engine is made to take, a chip-wide batch behind it, rolled back one by one.  Every state against the oracle's Statement and against the same script on
    the engine path alone."""
    snap, cfg, once, again, more = config0_batches()
    sc = once + again + more; a, b = len(once), len(once) + len(again)
    for what, calls, paths, steps in (
            ("wide then engine", [(BEGIN, 0, 0, 0), (APPLY, 0, 0, a), (APPLY, 0, a, b), (APPLY, 0, b, len(sc)), (ROLLBACK, 0, b, 0), (ROLLBACK, 0, 3, 0), (APPLY, 0, 3, a), (DISCARD, 0, 0, 0)],
             [WIDE, ENGINE, WIDE, WIDE, ENGINE, WIDE, WIDE],
             [("apply", 0, a), ("apply", a, b), ("apply", b, len(sc)), ("rollback", b), ("rollback", 3), ("apply", 3, a), ("discard",)]),
            ("engine then wide", [(BEGIN, 0, 0, 0), (APPLY, EP, 0, a), (APPLY, 0, b, len(sc)), (ROLLBACK, 0, a, 0), (APPLY, 0, b, len(sc)), (ROLLBACK, 0, 2, 0), (DISCARD, 0, 0, 0)],
             [ENGINE, WIDE, WIDE, WIDE, ENGINE, ENGINE], None)):
        res, _, _ = sim_script(snap, cfg, OA.make_ops(sc), calls, lanes=lanes)
        eng, _, _ = sim_script(snap, cfg, OA.make_ops(sc), [(k, (f | EP) if k in (APPLY, ROLLBACK, DISCARD) else f, lo, hi) for k, f, lo, hi in calls], lanes=lanes)
        assert [r.status for r in res] == [0] * len(calls) and [r.path for r in res[1:]] == paths, (what, [r.path for r in res[1:]])
        assert all(r.path == ENGINE for r in eng[1:])
        for k in range(len(calls)): same_all(res[k], eng[k], f"{what}: call {k} against the engine path alone")
        if steps:
            for k in range(len(steps)):
                r, st, nd, nodes = oracle_state(snap, cfg, _prefix_rows(sc, steps, k))
                OA.same_state(res[k + 1], np.array(st, np.int32), np.array(nd, np.int32), nodes, what=f"{what}: behind step {k}")
        same_readbacks(res[-1], res[0], f"{what}: the discard restores the read-backs")


# ---- (4) plugins on, exact sums
CUTS = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def allocate_case():
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    return snap, cfg, T.Oracle.run(snap, cfg, ("allocate",))


@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
@pytest.mark.parametrize("lanes", [256, 100, 1])
def test_allocate_in_chunks_rolled_back_to_every_checkpoint(allocate_case, lanes, engine):
    """the oracle's allocate (649 operations) applied in chunks with checkpoints at 1, 63, 64, 65 and 257 operations, rolled back to each: the read-backs, the shares among them,
    are those of the moment the checkpoint was taken and of a twin that applied only that prefix; the discard gives the fresh session's read-backs bit for bit"""
    snap, cfg, ref = allocate_case
    n = len(ref.ops); assert n == 649
    f = EP if engine else 0
    edges = [0] + CUTS + [n]
    calls = [(BEGIN, 0, 0, 0)] + [(APPLY, f, edges[i], edges[i + 1]) for i in range(len(edges) - 1)] + [(ROLLBACK, f, cp, 0) for cp in reversed(CUTS)] + [(DISCARD, f, 0, 0)]
    res, _, _ = sim_script(snap, cfg, OA.ref_ops(ref), calls, lanes=lanes)
    assert [r.status for r in res] == [0] * len(calls)
    want = ENGINE if engine else WIDE
    assert all(r.path == want for r in res[1:]), [r.path for r in res]
    assert [r.log_len for r in res] == [0] + edges[1:] + list(reversed(CUTS)) + [0]
    whole = res[len(edges) - 1]
    st = ref.pod_status.copy(); st[st == S["Binding"]] = S["Allocated"]  # nothing is committed
    OA.same_state(whole, st, ref.pod_node, ref.nodes, ref.shares_final, "the whole action, uncommitted")
    for k, cp in enumerate(reversed(CUTS)):
        same_readbacks(res[len(edges) + k], res[1 + CUTS.index(cp)], f"rolled back to {cp}")
    same_readbacks(res[-1], res[0], "discard")
    for k, cp in enumerate(reversed(CUTS)):  # a twin that applied only the prefix
        twin, _, _ = sim_script(snap, cfg, OA.ref_ops(ref), [(BEGIN, 0, 0, 0), (APPLY, f, 0, cp)], lanes=lanes)
        same_readbacks(res[len(edges) + k], twin[1], f"rolled back to {cp} against the twin")


def test_the_paths_agree_on_chunks_and_rollbacks(allocate_case):
    snap, cfg, ref = allocate_case
    calls = [(BEGIN, 0, 0, 0), (APPLY, 0, 0, 64), (APPLY, 0, 64, 257), (ROLLBACK, 0, 65, 0), (APPLY, 0, 65, 649), (ROLLBACK, 0, 1, 0)]
    w, _, _ = sim_script(snap, cfg, OA.ref_ops(ref), calls)
    e, _, _ = sim_script(snap, cfg, OA.ref_ops(ref), [(k, f | EP if k != BEGIN else 0, lo, hi) for k, f, lo, hi in calls])
    for k in range(len(calls)): same_all(w[k], e[k], f"call {k}")


@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_commit_is_ops_apply_of_the_surviving_operations(allocate_case, engine):
    """commit of the whole action: the oracle's state, Binding where the oracle committed; everything — hidden words included — as kai_ops_apply leaves it with the same
    operations as one Statement; the operations come back as they went in"""
    snap, cfg, ref = allocate_case
    f = EP if engine else 0
    ops = OA.ref_ops(ref); ops["stmt"] = 0
    res, _, _ = sim_script(snap, cfg, ops, [(BEGIN, 0, 0, 0), (APPLY, f, 0, 300), (APPLY, f, 300, 649), (ROLLBACK, f, 300, 0), (APPLY, f, 300, 649), (COMMIT, 0, 0, 0)])
    assert [r.status for r in res] == [0] * 6 and res[-1].path == (ENGINE if engine else WIDE) and res[-1].log_len == 0
    OA.same_state(res[-1], ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "committed")
    twin, _, _ = sim_script(snap, cfg, ops, [(OPS_APPLY, f, 0, 649)])
    assert twin[0].status == 0
    same_all(closed(res[-1]), closed(twin[0]), "commit against kai_ops_apply")
    got = res[-1].q.reshape(-1, 6)
    assert [tuple(r[:4]) for r in got.tolist()] == ref.ops and (got[:, 4] == 0).all() and got[:, 5].tolist() == list(range(649))


WIDE_VICTIM = OA.WIDE_VICTIM


@pytest.mark.parametrize("lanes", [256, 100, 1])
@pytest.mark.parametrize("seed,action,counts", WIDE_VICTIM, ids=[f"crowded{s}-{a}" for s, a, _ in WIDE_VICTIM])
def test_evictions_and_pipelines_rolled_back_and_committed(seed, action, counts, lanes):
    """a victim action's operations (evictions, pipelines, allocations): applied, rolled back to the middle and to nothing, applied again, committed — against the oracle's
    state, on both paths"""
    snap, cfg = crowded(seed)
    ref = T.Oracle.run(snap, cfg, (action,))
    n = len(ref.ops); m = n // 2
    ops = OA.ref_ops(ref); ops["stmt"] = 0
    out = {}
    for f in (0, EP):
        res, _, _ = sim_script(snap, cfg, ops, [(BEGIN, 0, 0, 0), (APPLY, f, 0, m), (APPLY, f, m, n), (ROLLBACK, f, m, 0), (ROLLBACK, f, 0, 0), (APPLY, f, 0, n), (COMMIT, 0, 0, 0)], lanes=lanes)
        assert [r.status for r in res] == [0] * 7 and all(r.path == (ENGINE if f else WIDE) for r in res[1:]), [r.path for r in res]
        same_readbacks(res[3], res[1], "rolled back to the middle"); same_readbacks(res[4], res[0], "rolled back to nothing")
        OA.same_state(res[-1], ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "committed")
        out[f] = res
    for k in range(7): same_all(out[0][k], out[EP][k], f"call {k}: wide against engine")
    twin, _, _ = sim_script(snap, cfg, ops, [(OPS_APPLY, 0, 0, n)], lanes=lanes)
    same_all(closed(out[0][-1]), closed(twin[0]), "commit against kai_ops_apply")


def test_rolled_back_evictions_do_not_keep_allocate_off_its_batch_path():
    """evictions applied and rolled back, allocations committed: the allocate action afterwards commits the same operations, on the same path (kai_action_stats.reserved[4]:
    actions on the batch path), as on a twin that took the allocations through kai_ops_apply — and as it would NOT with fast_ok lowered (the evictions committed)"""
    snap, cfg = crowded(5)
    st, nd = snap.arrays["pod_status"], snap.arrays["pod_node"]
    placed = np.nonzero((st == S["Running"]) & (nd >= 0))[0]
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    allocs = [o for o in ref.ops][:4]
    evicts = [(EVICT, int(p), int(nd[p])) for p in placed[:3]]
    assert len(allocs) == 4 and len(evicts) == 3
    ops = OA.make_ops(allocs + evicts)
    a, n = len(allocs), len(allocs) + len(evicts)
    for f in (0, EP):
        res, got, stats = sim_script(snap, cfg, ops, [(BEGIN, 0, 0, 0), (APPLY, f, a, n), (ROLLBACK, f, 0, 0), (APPLY, f, 0, a), (COMMIT, 0, 0, 0), (ACTION, 0, 0, 0)], batch=True)
        twin, want, tstats = sim_script(snap, cfg, ops, [(OPS_APPLY, f, 0, a), (ACTION, 0, 0, 0)], batch=True)
        assert [r.status for r in res] == [0] * 6
        assert tstats.reserved[4] == 1, "the twin's allocate takes the batch path (else this test shows nothing)"
        assert got == want and len(got) > 0 and stats.reserved[4] == tstats.reserved[4]
        same_readbacks(res[-1], twin[-1], "the allocate action behind the commit")
        low, _, lstats = sim_script(snap, cfg, ops, [(BEGIN, 0, 0, 0), (APPLY, f, 0, n), (COMMIT, 0, 0, 0), (ACTION, 0, 0, 0)], batch=True)
        assert lstats.reserved[4] == 0, "committed evictions do lower fast_ok"


# ---- (5) a precondition that fails in the middle of a Statement
def test_a_failing_precondition_leaves_the_statement_as_it_was(allocate_case):
    snap, cfg, ref = allocate_case
    st, nd = snap.arrays["pod_status"], snap.arrays["pod_node"]
    used = {o[1] for o in ref.ops}
    running = [int(p) for p in np.nonzero((st == S["Running"]) & (nd >= 0))[0] if p not in used]
    rows = list(ref.ops[:100]) + list(ref.ops[100:120]) + [(ALLOCATE, running[0], 0)] + list(ref.ops[120:140]) + [ref.ops[5]] + list(ref.ops[140:150]) + [(EVICT, ref.ops[150][1], ref.ops[150][2])] + list(ref.ops[100:130])
    ops = OA.make_ops(rows)
    for f in (0, EP):
        calls = [(BEGIN, 0, 0, 0), (APPLY, f, 0, 100),
                 (APPLY, f, 100, 141),   # a Running pod allocated at 120: the check finds it
                 (APPLY, f, 121, 152),   # a pod of the log allocated again at 141: only the walk over the shadow can tell
                 (APPLY, f, 142, 153),   # a Pending pod evicted at 152
                 (APPLY, f | abi.APPLY_CHECK_ONLY, 100, 120), (ROLLBACK, f, 50, 0), (APPLY, f, 50, 100), (APPLY, f, 153, 183)]
        res, _, _ = sim_script(snap, cfg, ops, calls)
        assert [(r.status, r.first_bad) for r in res[2:5]] == [(-6, 20), (-6, 20), (-6, 10)], [(r.status, r.first_bad) for r in res]
        for k in (2, 3, 4, 5): same_all(res[k], res[1], f"flags {f}: call {k} wrote nothing")
        assert res[5].status == 0 and res[5].log_len == 100
        assert [r.status for r in res[6:]] == [0, 0, 0] and [r.log_len for r in res[6:]] == [50, 100, 130]
        if not f: assert [r.path for r in res[6:]] == [WIDE, WIDE, WIDE], "pods that were rolled back are allocated again on the chip-wide path"
        same_readbacks(res[7], res[1], "applied again")


# ---- (6) queries while a Statement is open
def test_queries_see_the_tentative_state_and_leave_the_log():
    """kai_job_order and kai_subset_nodes, each on both its paths, kai_best_nodes and kai_ordered_nodes (k = 4) over all Pending pods, while a Statement is open: the answers of a twin that took the same operations through kai_ops_apply; the
    log and everything else is untouched (the tasks-to-allocate caches' validity is theirs to re-derive); a rollback still restores the read-backs"""
    import test_subset_nodes as SN
    snap, cfg = SN.synthetic(48, 2, 3)
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    n = min(len(ref.ops), 40); assert n >= 8
    ops = OA.ref_ops(ref, 0, n); ops["stmt"] = 0
    jobs = SN.topology_jobs(snap)
    J, P, SS = snap.n_jobs, snap.n_pods, snap.n_podsets
    queries = [(JOB_ORDER, 0, 0, 0), (JOB_ORDER, abi.JOB_ORDER_ENGINE_PATH, 0, 0), (SUBSET, 0, 0, len(jobs)), (SUBSET, abi.SUBSET_ENGINE_PATH, 0, len(jobs)),
               (BEST_NODES, 0, 0, 0), (ORDERED_NODES, 0, 4, 0)]  # the last two over all Pending pods
    NQ = len(queries)
    for f in (0, EP):
        res, _, _ = sim_script(snap, cfg, ops, [(BEGIN, 0, 0, 0), (APPLY, f, 0, n)] + queries + [(ROLLBACK, f, 0, 0)] + queries, jobs=jobs)
        twin, _, _ = sim_script(snap, cfg, ops, [(OPS_APPLY, f, 0, n)] + queries, jobs=jobs)
        fresh, _, _ = sim_script(snap, cfg, ops, queries, jobs=jobs)
        assert [r.status for r in res] == [0] * len(res) and [r.status for r in twin] == [0] * (1 + NQ)
        for k in range(NQ):
            assert len(res[2 + k].q) > 0 and np.array_equal(res[2 + k].q, twin[1 + k].q), f"query {k} while the Statement is open"
            assert np.array_equal(res[3 + NQ + k].q, fresh[k].q), f"query {k} behind the rollback"
            assert res[2 + k].path == twin[1 + k].path
        for k in (0, 2, 4, 5):
            assert not np.array_equal(res[2 + k].q, fresh[k].q), f"the applied operations change the answer of query {k} (else this test shows nothing)"
        def masked(h):
            h = h.copy(); h[4 * P + 4 * SS + 1: 4 * P + 4 * SS + 8 * J: 8] = 0; return h
        for k in range(NQ):
            same_readbacks(res[2 + k], res[1], f"query {k}")
            assert np.array_equal(masked(res[2 + k].hidden), masked(res[1].hidden)), f"query {k} touched the log or the hidden state"
        same_readbacks(res[2 + NQ], res[0], "the rollback behind the queries")


# ---- (7) the scene of the composed walk (tests/test_gpu_stmt.py runs the walk on the device)
def walk_scene():
    """two racks under one zone; rack A: two nodes with 2 free GPUs each; rack B: one node with 4.  A gang of a CPU-only task and a 3-GPU task that requires one rack.  (Tasks
    of which some use GPUs and some do not switch the topology plugin's representor accounting off: the domain check then sums resources, and rack A's 4 GPUs pass it.)"""
    rn = lambda rack, g, c: {"CPUMillis": c, "GPUs": g, "MaxTaskNum": 100, "Labels": {"zone": "zone1", "rack": rack}}
    nodes = {"node-a1": rn("rackA", 2, 8000), "node-a2": rn("rackA", 2, 8000), "node-b1": rn("rackB", 4, 64000)}
    jobs = [{"Name": "gang", "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": 1, "RootSubGroupSet": KAT._root("rack"),
             "Tasks": [{"State": "Pending", "RequiredGPUs": 0}, {"State": "Pending", "RequiredGPUs": 3}]}]
    case = {"Name": "walk", "Nodes": nodes, "Topologies": KAT.TOPO, "Queues": [{"Name": "q", "DeservedGPUs": 8}], "Jobs": jobs, "JobExpectedResults": {}}
    snap, cfg, _ = T.case_to_snapshot(case)
    cfg.plugins |= abi.PLUGINS["topology"]
    return snap, cfg


WALK_OPS = [(ALLOCATE, 0, 2, 0), (ALLOCATE, 1, 2, 0)]  # the oracle's allocate on walk_scene(): both pods on node-b1 (test_the_walks_scene_against_the_oracle)


@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
@pytest.mark.parametrize("lanes", [256, 100, 1])
def test_the_composed_walk(lanes, engine):
    """the scene is what the walk needs — subSetNodesFn offers rack A first and rack B second, the oracle's allocate rolls back and places both pods on rack B's node — and the
    walk with emulated lanes (tests/host_sim/stmt_sim.cpp sim_walk: begin; per node set of kai_subset_nodes a checkpoint; per task kai_ordered_nodes(k = 1) inside the set and
    apply; on an empty answer rollback and the next set; commit): rack A takes the CPU-only task and has no node for the 3-GPU task, so ONE operation is rolled back; the end is
    the oracle's operations and state, and what the allocate action gives on a twin"""
    import test_subset_nodes as SN
    snap, cfg = walk_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    assert ref.ops == WALK_OPS and ref.stats.rollbacks >= 1 and ref.stats.jobs_committed == 1
    assert SN.oracle_answer(snap, cfg, 0) == (0, [(0, 1), (2,)])
    res, _, _ = sim_script(snap, cfg, OA.make_ops([]), [(WALK, EP if engine else 0, 0, 0)], lanes=lanes)
    w = res[0]
    assert w.status == 0 and w.log_len == 0 and w.path == (ENGINE if engine else WIDE)
    assert w.q[:4].tolist() == [1, 2, 1, 2], "placed; two sets tried; the first had applied one operation when it was rolled back, the second took both"
    got = w.q[4:].reshape(-1, 6)
    assert [tuple(r[:4]) for r in got.tolist()] == ref.ops and (got[:, 4] == 0).all() and got[:, 5].tolist() == [0, 1]
    OA.same_state(w, ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "the walk against the oracle")
    twin, ops, _ = sim_script(snap, cfg, OA.make_ops([]), [(ACTION, 0, 0, 0)], lanes=lanes)
    assert ops == ref.ops
    same_readbacks(w, twin[0], "the walk against the allocate action")
