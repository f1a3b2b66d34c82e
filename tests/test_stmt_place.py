"""kai_stmt_place (whole gangs placed on their node sets in one call, inside the open Statement) without a GPU.

 - the exports, the ABI structs, the header's text;
 - arguments under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp): every refusal is made before the first write and leaves
   the device image and the Statement as they were; a warm call is one upload, two launches, no allocation;
 - the two kernel bodies (kai_stmt_place.hpp) run with emulated lanes by tests/host_sim/stmt_place_sim.cpp on a session of the host simulation, in both apply modes, in
   workgroups of 256 and 64 lanes: every case against THE LOOP OVER THE EXISTING CALLS the contract names (checkpoint; kai_ordered_nodes_scored with k = 1 and kai_stmt_apply
   of one operation per task; kai_stmt_rollback) — read-backs, the hidden state and the log's records byte for byte — and, where the scene is the allocate action's, against
   the oracle and the action on a twin.
The parity claim on the device is tests/test_gpu_stmt_place.py."""
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
import test_stmt as TS
import test_subset_nodes as SN
import test_topo_scores as TSC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
S = abi.POD_STATUS
ALLOCATE, PIPELINE, EVICT, WIDE, ENGINE, EP = TS.ALLOCATE, TS.PIPELINE, TS.EVICT, TS.WIDE, TS.ENGINE, TS.EP
BEGIN, APPLY, ROLLBACK, DISCARD, COMMIT, ACTION, OPS_APPLY = TS.BEGIN, TS.APPLY, TS.ROLLBACK, TS.DISCARD, TS.COMMIT, TS.ACTION, TS.OPS_APPLY
ORDERED_NODES, PLACE, LOOP = 10, 12, 13  # kai_spsim_run's kinds (tests/host_sim/stmt_place_sim.cpp)
PO = 0x4  # KAI_PLACE_PIPELINE_ONLY
PLACED, NO_FIT = 0, 1
G_DT = np.dtype([("first_task", "<i4"), ("n_tasks", "<i4"), ("first_set", "<i4"), ("n_sets", "<i4"), ("scores", "<i4"), ("pad", "<i4")])
MODES = [(0, 256), (0, 64), (EP, 256), (EP, 64)]  # (apply mode, emulated lanes)
MODE_IDS = ["wide-256", "wide-64", "engine-256", "engine-64"]


def test_exports_and_struct_sizes():
    lib = T.pkg.load_library()
    assert "kai_stmt_place" in T.pkg.core.EXPORTS and hasattr(lib, "kai_stmt_place")
    Gg, A, Pp = abi.KaiPlaceGang, abi.KaiPlaceAnswer, abi.KaiPlaceParams
    assert C.sizeof(Pp) == 8 and [f[0] for f in Pp._fields_] == ["version", "flags"]
    assert C.sizeof(Gg) == 24 and [f[0] for f in Gg._fields_] == ["first_task", "n_tasks", "first_set", "n_sets", "scores", "pad"]
    assert C.sizeof(A) == 32 and (A.status.offset, A.set.offset, A.sets_tried.offset, A.pad.offset, A.first_op.offset, A.n_ops.offset) == (0, 4, 8, 12, 16, 24)
    assert (abi.PLACE_VERSION, abi.PLACE_PIPELINE_ONLY, abi.PLACE_PLACED, abi.PLACE_NO_FIT) == (1, 4, 0, 1) and abi.APPLY_ENGINE_PATH == 2
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    for text in ("#define KAI_PLACE_VERSION 1u", "#define KAI_PLACE_PIPELINE_ONLY 0x4u", "enum { KAI_PLACE_PLACED = 0, KAI_PLACE_NO_FIT = 1 };",
                 "typedef struct kai_place_params { uint32_t version; uint32_t flags; } kai_place_params;", "} kai_place_gang;", "} kai_place_answer;",
                 "int kai_stmt_place(kai_core* core, const kai_place_params* params,"):
        assert text in hdr, text
    assert hasattr(T.pkg.core.Statement, "place")


# ---------------------------------------------------------------------------------------------- the host side under the host-only library
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
Op, Res, Gg, An, Pp, Sr = abi.KaiOp, abi.KaiStmtResult, abi.KaiPlaceGang, abi.KaiPlaceAnswer, abi.KaiPlaceParams, abi.KaiTopoScoreRow
I32 = C.POINTER(C.c_int32)
lib.kai_stmt_begin.argtypes = [C.c_void_p, C.c_uint32]
lib.kai_stmt_apply.argtypes = [C.c_void_p, C.POINTER(Op), C.c_int64, C.c_uint32, C.POINTER(Res)]
lib.kai_stmt_checkpoint.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
lib.kai_stmt_discard.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Res)]
lib.kai_stmt_place.argtypes = [C.c_void_p, C.POINTER(Pp), C.POINTER(Gg), C.c_int32, I32, C.c_int32, I32, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(Sr), C.POINTER(C.c_uint8), C.c_int32,
                               C.POINTER(An), I32, C.POINTER(Op), C.c_int64, C.POINTER(C.c_int64), C.POINTER(Res)]
snap, cfg, _ = pkg.synth.config(1, 0.3)
cfg = abi.copy_config(cfg); cfg.now_ns = 10**9
P, N, J = snap.n_pods, snap.n_nodes, snap.n_jobs
W = (N + 31) // 32
D = int(snap.arrays["domain_level"].shape[0]) if "domain_level" in snap.arrays else 0
TL = int(snap.arrays["node_domain"].shape[0]) if "node_domain" in snap.arrays else 0
pending = [int(p) for p in np.nonzero(snap.arrays["pod_status"] == abi.POD_STATUS["Pending"])[0][:8]]
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def diff(a, b): return dict(allocations=b[1] - a[1], live_bytes=b[2] - a[2], launches=b[3] - a[3], h2d=b[4] - a[4], memsets=b[7] - a[7], pinned=b[8] - a[8])
def checkpoint(h):
    cp = C.c_int64(-7); rc = lib.kai_stmt_checkpoint(h, C.byref(cp)); return [rc, cp.value]
SENT = 0x5a5a5a5a
def place(h, gangs=((0, 2, 0, 2, -1, 0), (2, 3, 1, 1, -1, 0)), tasks=None, sets=(0, -1), rows=2, version=1, flags=0, n_gangs=None, n_tasks=None, n_sets=None, cap=None, null=(),
          srows=(), dec=None, n_srows=None, res=True, params=True):
    tasks = pending[:5] if tasks is None else tasks
    ga = (Gg * max(len(gangs), 1))(*[Gg(*g) for g in gangs]); ta = (C.c_int32 * max(len(tasks), 1))(*tasks); sa = (C.c_int32 * max(len(sets), 1))(*sets)
    words = (C.c_uint32 * max(rows * W, 1))(*([0xffffffff] * (rows * W)))
    sr = (Sr * max(len(srows), 1))(*[Sr(*x) for x in srows]); dc = (C.c_uint8 * max(len(srows) * max(D, 1), 1))(*(dec if dec is not None else [255] * (len(srows) * max(D, 1))))
    an = (An * max(len(gangs), 1))(); fa = (C.c_int32 * max(len(sets), 1))(*([SENT] * max(len(sets), 1))); ops = (Op * max(len(tasks), 1))(); ops[0].pod = SENT
    n = C.c_int64(-7); r = Res(123, 45, 67, 89); pp = Pp(version, flags)
    rc = lib.kai_stmt_place(h, C.byref(pp) if params else None, None if "gangs" in null else ga, len(gangs) if n_gangs is None else n_gangs, None if "tasks" in null else ta, len(tasks) if n_tasks is None else n_tasks,
                            None if "sets" in null else sa, len(sets) if n_sets is None else n_sets, None if "rows" in null else words, rows,
                            None if "srows" in null else sr, None if "dec" in null else dc, len(srows) if n_srows is None else n_srows,
                            None if "answers" in null else an, None if "fail_at" in null else fa, None if "ops" in null else ops, len(tasks) if cap is None else cap, C.byref(n), C.byref(r) if res else None)
    return [rc, r.first_bad, r.log_len, r.path, n.value, fa[0] == SENT and ops[0].pod == SENT]
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
res["before_open"] = place(h)[0]
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
res["without_begin"] = place(h)[0]
assert lib.kai_stmt_begin(h, 1) == 0
arr = (Op * 1)(Op(0, 0, pending[7], 0, -1, 0, 0)); r0 = Res()
assert lib.kai_stmt_apply(h, arr, 1, 0, C.byref(r0)) == 0   # one record lies under everything that follows
img1 = image()
bad = {}
bad["null_params"] = place(h, params=False)
bad["version"] = place(h, version=2)
bad["flags"] = place(h, flags=1)
bad["flags_high"] = place(h, flags=8)
bad["gang_pad"] = place(h, gangs=((0, 2, 0, 2, -1, 7), (2, 3, 1, 1, -1, 0)))
bad["null_gangs"] = place(h, null=("gangs",))
bad["null_tasks"] = place(h, null=("tasks",))
bad["null_sets"] = place(h, null=("sets",))
bad["null_rows"] = place(h, null=("rows",))
bad["null_answers"] = place(h, null=("answers",))
bad["null_ops"] = place(h, null=("ops",))
bad["null_score_rows"] = place(h, srows=((0, 1),), null=("srows",))
bad["null_deciles"] = place(h, srows=((0, 1),), null=("dec",))
bad["negative_gangs"] = place(h, n_gangs=-1)
bad["negative_tasks"] = place(h, n_tasks=-1)
bad["negative_sets"] = place(h, n_sets=-1)
bad["negative_cap"] = place(h, cap=-1)
bad["task_range"] = place(h, gangs=((0, 2, 0, 2, -1, 0), (2, 4, 1, 1, -1, 0)))
bad["task_range_negative"] = place(h, gangs=((-1, 2, 0, 2, -1, 0),))
bad["set_range"] = place(h, gangs=((0, 2, 0, 3, -1, 0),))
bad["no_tasks"] = place(h, gangs=((0, 0, 0, 2, -1, 0),))
bad["no_sets"] = place(h, gangs=((0, 2, 0, 0, -1, 0),))
bad["gangs_share_tasks"] = place(h, gangs=((0, 2, 0, 2, -1, 0), (1, 3, 1, 1, -1, 0)))
bad["pod_negative"] = place(h, tasks=pending[:4] + [-1])
bad["pod_too_large"] = place(h, tasks=pending[:4] + [P])
bad["row_too_large"] = place(h, sets=(2, -1))
bad["row_below"] = place(h, sets=(0, -2))
bad["scores_too_large"] = place(h, gangs=((0, 2, 0, 2, 0, 0),))
bad["scores_below"] = place(h, gangs=((0, 2, 0, 2, -2, 0),))
bad["level_row"] = place(h, gangs=((0, 2, 0, 2, 0, 0),), srows=((TL, 1),))
bad["level_row_below"] = place(h, gangs=((0, 2, 0, 2, 0, 0),), srows=((-3, 0),))
bad["pod_twice"] = place(h, tasks=pending[:4] + [pending[1]])
if D > 0: bad["decile"] = place(h, gangs=((0, 2, 0, 2, 0, 0),), srows=((0, 1),), dec=[11] + [255] * (D - 1))
res["bad"] = bad
cap = {}
cap["ops_cap"] = place(h, cap=4)
cap["work"] = place(h, gangs=((0, 5, 0, 1 << 18, -1, 0),), sets=[-1] * (1 << 18))
res["capacity"] = cap
res["empty"] = place(h, gangs=(), tasks=(), sets=(), rows=0)
res["image_unchanged"] = image() == img1
res["still_open"] = checkpoint(h)
# good calls: what each costs on the device (the kernels of the host-only library do nothing: the verdict that comes back is the one that was sent: no task refused, the log as long as it was)
i0 = image(); res["first"] = place(h); i1 = image(); res["warm"] = place(h, flags=4, res=False)[0]; i2 = image()
res["first_cost"] = diff(i0, i1); res["warm_cost"] = diff(i1, i2)
res["engine"] = place(h, flags=2); res["after"] = checkpoint(h)
many = (Op * (2 * P + 28))(*[Op(0, 0, pending[6], 0, -1, 0, 0)] * (2 * P + 28))   # (the host-only library's check kernel does nothing: the log just grows)
assert lib.kai_stmt_apply(h, many, 2 * P + 28, 0, C.byref(r0)) == 0
i3 = image(); res["log_room"] = place(h); res["log_room_image_unchanged"] = image() == i3; res["log_room_after"] = checkpoint(h)
r1 = Res(); res["discard"] = lib.kai_stmt_discard(h, 0, C.byref(r1)); res["after_discard"] = place(h)[0]
lib.kai_core_destroy(h)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["sharded"] = place(h2)[0]
lib.kai_core_destroy(h2)
snap3, cfg3, _ = pkg.synth.config(1, 0.2); pkg.synth.add_fractions(snap3, 7, frac=0.3)
h3 = C.c_void_p(); st3 = snap3.as_struct()
assert lib.kai_core_create(C.byref(cfg3), 1, None, C.byref(h3)) == 0 and lib.kai_session_open(h3, C.byref(st3)) == 0
img3 = image()
res["shared"] = place(h3)[0]; res["shared_image_unchanged"] = image() == img3
lib.kai_core_destroy(h3)
print(json.dumps(res))
'''


def test_arguments_and_refusals(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["before_open"] == -6 and out["without_begin"] == -6, "KAI_ERR_STATE without an open session / an open Statement"
    assert len(out["bad"]) >= 32
    for k, v in out["bad"].items():
        assert v[0] == -1 and v[2] == 1 and v[5], (k, v)  # KAI_ERR_INVALID_ARG, the log as long as it was, the outputs untouched
    for k, v in out["capacity"].items():
        assert v[0] == -4 and v[2] == 1 and v[5], (k, v)
    assert out["empty"][:5] == [0, -1, 1, 0, 0], "n_gangs == 0: KAI_OK without a device call"
    assert out["image_unchanged"], "a refused or empty call allocated or wrote device memory"
    assert out["still_open"] == [0, 1], "the Statement stays open with its log as it was"
    assert out["first"][:5] == [0, -1, 1, WIDE, 0] and out["warm"] == 0 and out["engine"][:5] == [0, -1, 1, ENGINE, 0]
    fc = out["first_cost"]  # the first call of a handle allocates its scratch and staging
    assert (fc["allocations"], fc["launches"], fc["h2d"], fc["memsets"]) == (1, 2, 1, 0) and fc["pinned"] > 0, fc
    assert out["warm_cost"] == dict(allocations=0, live_bytes=0, launches=2, h2d=1, memsets=0, pinned=0), out["warm_cost"]
    assert out["after"] == [0, 1] and out["discard"] == 0 and out["after_discard"] == -6
    assert out["log_room"][0] == -4 and out["log_room"][5] and out["log_room_image_unchanged"] and out["log_room_after"][0] == 0, "KAI_ERR_CAPACITY: the log's length plus n_tasks above 2 n_pods + 32"
    assert out["sharded"] == -5, "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["shared"] == -5 and out["shared_image_unchanged"], "KAI_ERR_UNSUPPORTED in a session with shared-GPU requests, before the first device call"


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "stmt_place_sim.cpp")


def sim_lib():
    so = os.path.join(ROOT, "tests", "host_sim", "libstmtplacesim.so")
    deps = glob.glob(os.path.join(ROOT, "tests", "host_sim", "*.?pp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_spsim_run.restype = C.c_int; lib.kai_spsim_set.restype = C.c_int
    return lib


def words_of(rows, N):
    """node sets (index lists or boolean masks) -> uint32 [len(rows), ceil(N / 32)]"""
    w = np.zeros((max(len(rows), 1), max((N + 31) // 32, 1)), np.uint32)
    for s, ns in enumerate(rows):
        ns = np.asarray(ns)
        idx = np.nonzero(ns)[0] if ns.dtype == np.bool_ else ns.astype(np.int64).ravel()
        np.bitwise_or.at(w[s], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return w


def flatten(gangs):
    """gangs: (pods, sets[, scores]) -> the kai_place_gang records, tasks, sets"""
    gv = np.zeros(max(len(gangs), 1), G_DT); tasks, sets = [], []
    for g, gang in enumerate(gangs):
        gv[g] = (len(tasks), len(gang[0]), len(sets), len(gang[1]), gang[2] if len(gang) > 2 else -1, 0)
        tasks += [int(p) for p in gang[0]]; sets += [int(s) for s in gang[1]]
    return gv, np.array(tasks + [0], np.int32), np.array(sets + [0], np.int32), len(tasks), len(sets)


def place_script(snap, cfg, calls, gangs=(), rows=(), score_rows=None, deciles=None, ops=(), lanes=256, batch=False):
    """calls: (kind, flags, lo, hi) tuples (tests/host_sim/stmt_place_sim.cpp kai_spsim_run; PLACE and LOOP take the gangs [lo, hi)) -> as TS.sim_script: per call a Result,
    the operations of the script's actions, the action statistics.  A PLACE / LOOP call's Result also has answers [(status, set, sets_tried, first_op, n_ops)], fail_at (per
    entry of the sets of ALL gangs), placed [(kind, pod, node, job, stmt, seq)]."""
    lib = sim_lib()
    s = snap.as_struct()
    P, Q, N, J = snap.n_pods, max(snap.n_queues, 1), max(snap.n_nodes, 1), snap.n_jobs
    gv, tv, sv, n_t, n_s = flatten(gangs)
    words = np.ascontiguousarray(words_of(rows, snap.n_nodes))
    D = int(snap.arrays["domain_level"].shape[0]) if "domain_level" in snap.arrays else 0
    n_sr = 0 if score_rows is None else len(score_rows)
    sr = np.ascontiguousarray(score_rows, dtype=TSC.R_DT) if n_sr else np.zeros(1, TSC.R_DT)
    dc = np.ascontiguousarray(deciles, dtype=np.uint8) if n_sr else np.zeros(1, np.uint8)
    assert lib.kai_spsim_set(gv.ctypes.data_as(C.c_void_p), C.c_int32(len(gangs)), tv.ctypes.data_as(C.c_void_p), C.c_int32(n_t), sv.ctypes.data_as(C.c_void_p), C.c_int32(n_s),
                             words.ctypes.data_as(C.c_void_p), C.c_int32(len(rows)), C.c_int32(words.shape[1]), sr.ctypes.data_as(C.c_void_p), dc.ctypes.data_as(C.c_void_p), C.c_int32(n_sr), C.c_int32(D)) == 0
    ops = np.ascontiguousarray(ops if len(ops) else OA.make_ops([]), dtype=OA.OP_DT)
    ca = np.array([tuple(c) for c in calls], dtype=TS.CALL_DT); K = len(ca)
    ret = np.zeros(K, TS.RET_DT)
    hs = 4 * P + 4 * snap.n_podsets + 8 * J + 8 + TS.N_TAIL + 10 * (2 * P + 32)
    qs = 6 * (2 * P + 32) + 64 + 5 * len(gangs) + n_s + 3 * P
    st, nd = np.zeros((K, P), np.int32), np.zeros((K, P), np.int32)
    sh = (abi.KaiQueueShare * (K * Q))(); ns = (abi.KaiNodeState * (K * N))()
    hid, qo = np.zeros((K, hs), np.int32), np.zeros((K, qs), np.int32)
    cap = max(64, 8 * P); out = (abi.KaiOp * cap)(); n_out = C.c_int64(0); stats = abi.KaiActionStats()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.kai_spsim_run(C.byref(cfg), C.byref(s), C.c_int(int(batch)), ops.ctypes.data_as(C.c_void_p), C.c_int64(len(ops)), ca.ctypes.data_as(C.c_void_p), C.c_int(K), C.c_int(lanes),
                           ret.ctypes.data_as(C.c_void_p), ip(st), ip(nd), sh, ns, ip(hid), C.c_int64(hs), ip(qo), C.c_int64(qs), out, C.c_int64(cap), C.byref(n_out), C.byref(stats))
    assert rc == 0, f"kai_spsim_run rc={rc}"
    shares = TS._rows(sh, K, Q, [f[0] for f in abi.KaiQueueShare._fields_], 3)
    nodes = TS._rows(ns, K, N, [f[0] for f in abi.KaiNodeState._fields_], snap.n_res)
    res = []
    for k in range(K):
        r = T.Result(status=int(ret[k]["status"]), path=int(ret[k]["path"]), first_bad=int(ret[k]["first_bad"]), log_len=int(ret[k]["log_len"]), pod_status=st[k], pod_node=nd[k],
                     nodes=nodes[k], shares=shares[k], hidden=hid[k, : ret[k]["n_hidden"]].copy(), q=qo[k, : ret[k]["n_q"]].copy())
        if ca[k]["kind"] in (PLACE, LOOP) and r.status == 0 and len(r.q):
            g = int(ca[k]["hi"] - ca[k]["lo"])
            r.answers = [tuple(x) for x in r.q[: 5 * g].reshape(g, 5).tolist()]
            r.fail_at = r.q[5 * g: 5 * g + n_s].tolist()
            r.placed = [tuple(x) for x in r.q[5 * g + n_s:].reshape(-1, 6).tolist()]
        res.append(r)
    return res, [(o.kind, o.pod, o.node, o.job) for o in out[: n_out.value]], stats


def against_the_loop(snap, cfg, head, tail, n_gangs, flags, lanes, **data):
    """the script head + [PLACE over all gangs] + tail against head + [LOOP over all gangs] + tail: every call's status, path, log length and output, the read-backs, the hidden
    state and the log's records.  -> (the place script's results, the loop script's)"""
    a, _, _ = place_script(snap, cfg, head + [(PLACE, flags, 0, n_gangs)] + tail, lanes=lanes, **data)
    b, _, _ = place_script(snap, cfg, head + [(LOOP, flags, 0, n_gangs)] + tail, lanes=lanes, **data)
    for k in range(len(a)):
        assert (a[k].status, a[k].log_len, a[k].first_bad) == (b[k].status, b[k].log_len, b[k].first_bad), (k, a[k].status, b[k].status, a[k].log_len, b[k].log_len)
        assert a[k].status == 0, (k, a[k].status)
        assert a[k].path == b[k].path, (k, a[k].path, b[k].path)
        assert np.array_equal(a[k].q, b[k].q), f"call {k}: the outputs differ: {a[k].q[:40].tolist()} / {b[k].q[:40].tolist()}"
        TS.same_all(a[k], b[k], f"call {k} against the loop over the existing calls")
    return a, b


# ---- (2) the scene of the composed walk
@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
def test_the_walks_scene_in_one_call(flags, lanes):
    """tests/test_stmt.py walk_scene(): rack A takes the CPU-only task and has no node for the 3-GPU task, rack B takes both — one call instead of the walk's six"""
    snap, cfg = TS.walk_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    assert ref.ops == TS.WALK_OPS and SN.oracle_answer(snap, cfg, 0) == (0, [(0, 1), (2,)])
    data = dict(gangs=[([0, 1], [0, 1])], rows=[(0, 1), (2,)])
    a, _ = against_the_loop(snap, cfg, [(BEGIN, 0, 0, 0)], [(COMMIT, 0, 0, 0)], 1, flags, lanes, **data)
    p = a[1]
    assert p.answers == [(PLACED, 1, 2, 0, 2)] and p.fail_at == [1, 2] and p.path == (ENGINE if flags else WIDE) and p.log_len == 2
    assert [x[:4] for x in p.placed] == TS.WALK_OPS and [x[4:] for x in p.placed] == [(0, 0), (0, 1)]
    got = a[2].q.reshape(-1, 6)
    assert [tuple(r[:4]) for r in got.tolist()] == ref.ops and a[2].path == (ENGINE if flags else WIDE)
    OA.same_state(a[2], ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "one call and a commit against the oracle")
    twin, ops, _ = place_script(snap, cfg, [(ACTION, 0, 0, 0)], lanes=lanes)
    assert ops == ref.ops
    TS.same_readbacks(a[2], twin[0], "one call and a commit against the allocate action")


# ---- (3) state dependence inside a gang
def binpack_scene(N):
    snap, cfg = SN.synthetic(48, 2, 3) if N == 48 else SN.synthetic(N, 2, 3, seed=9)
    assert cfg.gpu_strategy == abi.BINPACK
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    pend = [o[1] for o in ref.ops if o[0] == ALLOCATE]  # Pending pods the session has room for: the oracle's allocate places them
    assert len(pend) >= 12
    return snap, cfg, pend


@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", [48, 70])
def test_a_task_sees_what_its_predecessors_took(N, flags, lanes):
    """a bin-pack session; a gang of Pending GPU pods with a first set too small for it (rolled back) and a second set that crosses word and stride boundaries: the tasks fill
    more than one node, and at least one of them lands elsewhere than kai_ordered_nodes puts it at the entry state (asked through the loop, one task a gang, rolled back)"""
    snap, cfg, pend = binpack_scene(N)
    gang = pend[:10]
    first = [o[2] for o in T.Oracle.run(snap, cfg, ("allocate",)).ops if o[1] == gang[0]]  # a node that takes the first task, and not the whole gang
    small, big = first, [n for n in range(N) if n not in (0, 31, 64)]  # 70 nodes: 67 of them, past a stride of 64 lanes, not a multiple of 32 or 64
    data = dict(gangs=[(gang, [0, 1])] + [([p], [1]) for p in gang], rows=[small, big])
    a, _ = against_the_loop(snap, cfg, [(BEGIN, 0, 0, 0)], [(ROLLBACK, flags & EP, 0, 0), (DISCARD, 0, 0, 0)], 1, flags, lanes, **data)
    p = a[1]
    assert p.answers[0][:3] == (PLACED, 1, 2) and 1 <= p.fail_at[0] < len(gang) and p.fail_at[1] == len(gang), (p.answers, p.fail_at[:2])
    nodes = [x[2] for x in p.placed]
    assert len(set(nodes)) > 1, "the gang's tasks take more than one node"
    calls = [(BEGIN, 0, 0, 0)]
    for i in range(len(gang)): calls += [(LOOP, 0, 1 + i, 2 + i), (ROLLBACK, 0, 0, 0)]
    e, _, _ = place_script(snap, cfg, calls, lanes=lanes, **data)
    entry = [e[1 + 2 * i].placed[0][2] if e[1 + 2 * i].placed else -1 for i in range(len(gang))]
    assert any(x != y for x, y in zip(nodes, entry)), "no task's node differs from the entry state's answer: the scene shows nothing"
    TS.same_readbacks(a[2], a[0], "the rollback of the call's operations")


# ---- (4) a gang no set takes
@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
def test_a_gang_no_set_takes_leaves_nothing(flags, lanes):
    snap, cfg = TS.walk_scene()
    data = dict(gangs=[([0, 1], [0, 1])], rows=[(0, 1), (0,)], ops=OA.make_ops([(ALLOCATE, 0, 0), (ALLOCATE, 1, 2)]))
    a, _ = against_the_loop(snap, cfg, [(BEGIN, 0, 0, 0)], [(APPLY, 0, 0, 2)], 1, flags, lanes, **data)
    assert a[1].answers == [(NO_FIT, -1, 2, 0, 0)] and a[1].fail_at == [1, 1] and a[1].placed == [] and a[1].log_len == 0
    TS.same_readbacks(a[1], a[0], "a gang no set takes: the read-backs as before the call")
    assert a[2].path == WIDE and a[2].log_len == 2, "kai_stmt_apply of the same pods afterwards takes the chip-wide path"


# ---- (5) three gangs, the middle one failing on its queue's limit
def limit_scene():
    """four 4-GPU nodes; a queue limited to 6 GPUs; six Pending 2-GPU pods"""
    nodes = {f"n{i}": {"CPUMillis": 64000, "GPUs": 4, "MaxTaskNum": 100} for i in range(4)}
    jobs = [{"Name": f"j{i}", "Priority": 50, "QueueName": "q", "RequiredGPUsPerTask": 2, "Tasks": [{"State": "Pending"}]} for i in range(6)]
    case = {"Name": "limit", "Nodes": nodes, "Queues": [{"Name": "q", "DeservedGPUs": 4, "MaxAllowedGPUs": 6}], "Jobs": jobs, "JobExpectedResults": {}}
    snap, cfg, _ = T.case_to_snapshot(case)
    cfg.plugins |= abi.PLUGINS["predicates"]  # the task's own capacity check (capacity_policy.go:51-61) is the predicates plugin's first step
    return snap, cfg


@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
def test_three_gangs_the_middle_one_fails(flags, lanes):
    """gang 0 takes 4 of the queue's 6 GPUs; gang 1's second task is over the queue's capacity on every set (fail_at = its index), its first task's operation goes; gang 2
    sees gang 0's placements (bin-packing puts it on a node gang 0 used) and nothing of gang 1's (it is still under the limit)"""
    snap, cfg = limit_scene()
    assert cfg.gpu_strategy == abi.BINPACK
    data = dict(gangs=[([0, 1], [0]), ([2, 3, 4], [1, -1]), ([5], [-1])], rows=[(0, 1), (2, 3)])
    a, _ = against_the_loop(snap, cfg, [(BEGIN, 0, 0, 0)], [(COMMIT, 0, 0, 0)], 3, flags, lanes, **data)
    p = a[1]
    assert p.answers == [(PLACED, 0, 1, 0, 2), (NO_FIT, -1, 2, 2, 0), (PLACED, 0, 1, 2, 1)], p.answers
    assert p.fail_at == [2, 1, 1, 1] and [x[1] for x in p.placed] == [0, 1, 5] and [x[5] for x in p.placed] == [0, 1, 2]
    assert p.placed[0][2] == p.placed[1][2] and p.placed[2][2] in (0, 1) and p.placed[2][2] != p.placed[0][2], "bin-packing: gang 0 fills one node of its set; gang 2 goes beside it"
    assert (p.pod_status[[2, 3, 4]] == S["Pending"]).all()


# ---- (6) pipelines
@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("seed,action,counts", OA.WIDE_VICTIM, ids=[f"crowded{s}-{a}" for s, a, _ in OA.WIDE_VICTIM])
def test_tasks_placed_on_released_room_are_pipelined(seed, action, counts, flags, lanes):
    """a victim action's evictions applied in the Statement; the pods the oracle pipelined, placed over all nodes: they come back as KAI_OP_PIPELINE, on the room the evictions
    released; with KAI_PLACE_PIPELINE_ONLY every operation is a pipeline"""
    snap, cfg = crowded(seed)
    ref = T.Oracle.run(snap, cfg, (action,))
    ev = [o for o in ref.ops if o[0] == EVICT]; pods = [o[1] for o in ref.ops if o[0] == PIPELINE]
    assert len(ev) == counts[0] and len(pods) == counts[1]
    data = dict(gangs=[([p], [-1]) for p in pods], ops=OA.make_ops(ev))
    head = [(BEGIN, 0, 0, 0), (APPLY, flags & EP, 0, len(ev))]
    a, _ = against_the_loop(snap, cfg, head, [(ROLLBACK, flags & EP, len(ev), 0), (COMMIT, 0, 0, 0)], len(pods), flags, lanes, **data)
    kinds = [x[0] for x in a[2].placed]
    assert PIPELINE in kinds, f"no task was pipelined ({a[2].answers}): the scene shows nothing"
    assert [x[5] for x in a[2].placed] == list(range(len(ev), len(ev) + len(kinds))), "seq is the position in the log"
    TS.same_readbacks(a[3], a[1], "rolled back to the evictions")
    b, _ = against_the_loop(snap, cfg, head, [(COMMIT, 0, 0, 0)], len(pods), flags | PO, lanes, **data)
    assert b[2].placed and all(x[0] == PIPELINE for x in b[2].placed)


# ---- (7) scores
@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
def test_a_scored_gang_lands_where_the_allocate_action_puts_it(flags, lanes):
    """tests/test_topo_scores.py gang_scene(): the zone is the only set and the preferred level's scores decide which rack fills first; one call with the score row places the
    gang pod for pod where the oracle's allocate does; without the row it starts on another rack"""
    snap, cfg = TSC.gang_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    gang = snap.job_names.index("gang")
    mine = [o for o in ref.ops if o[3] == gang]
    assert len(mine) == 6
    with TSC.Sim(snap, cfg) as sim:
        r = sim.subset([gang])
    assert r.call_status == 0 and r.ans["n_sets"][0] == 1 and r.score_rows["level_row"][0] == 1
    pods = [o[1] for o in mine]
    data = dict(gangs=[(pods, [0], 0)], rows=[r.masks[0]], score_rows=r.score_rows, deciles=r.deciles)
    a, _ = against_the_loop(snap, cfg, [(BEGIN, 0, 0, 0)], [(COMMIT, 0, 0, 0)], 1, flags, lanes, **data)
    assert [x[:4] for x in a[1].placed] == mine, "pod for pod where the oracle's allocate puts the gang"
    OA.same_state(a[2], ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "the scored gang, committed, against the oracle")
    u, _, _ = place_script(snap, cfg, [(BEGIN, 0, 0, 0), (PLACE, flags, 0, 1)], gangs=[(pods, [0])], rows=[r.masks[0]], lanes=lanes)
    assert u[1].placed[0][2] != mine[0][2], "without the score row the gang starts elsewhere (else the scores show nothing)"


# ---- (8) seams
@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
def test_the_calls_records_and_kai_stmt_applys_lie_on_one_log(flags, lanes):
    """records of kai_stmt_apply under the call's own, more of them on top; rolled back to every checkpoint on both of kai_stmt_rollback's paths, and committed: a twin that
    made the loop's calls instead gives the same states, logs and operations"""
    snap, cfg, pend = binpack_scene(48)
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    under = [o for o in ref.ops if o[0] == ALLOCATE][:5]
    used = {o[1] for o in under}
    free = [p for p in pend if p not in used]
    gangs = [(free[0:3], [0, -1]), (free[3:5], [-1]), (free[5:9], [1, 0, -1])]
    over = [(PIPELINE, free[9], 3), (ALLOCATE, free[10], 4)]
    ops = OA.make_ops(under + over)
    rows = [list(range(5, 40)), [2, 3]]
    head = [(BEGIN, 0, 0, 0), (APPLY, flags & EP, 0, 5)]
    for rb in (0, EP):
        tail = [(APPLY, flags & EP, 5, 7)]
        probe, _, _ = place_script(snap, cfg, head + [(PLACE, flags, 0, 3)], gangs=gangs, rows=rows, ops=ops, lanes=lanes)
        n = probe[2].log_len
        assert n > 5 + 3, "the call left records of its own"
        tail += [(ROLLBACK, rb, n + 1, 0), (ROLLBACK, rb, n - 1, 0), (ROLLBACK, rb, 6, 0), (ROLLBACK, rb, 5, 0), (ROLLBACK, rb, 2, 0), (COMMIT, 0, 0, 0)]
        a, _ = against_the_loop(snap, cfg, head, tail, 3, flags, lanes, gangs=gangs, rows=rows, ops=ops)
        assert [r.log_len for r in a[3:]] == [n + 2, n + 1, n - 1, 6, 5, 2, 0]
        if not flags and not rb: assert all(r.path == WIDE for r in a[1:]), [r.path for r in a]
        TS.same_readbacks(a[7], a[1], "rolled back under the call's records")
    c, _ = against_the_loop(snap, cfg, head, [(APPLY, flags & EP, 5, 7), (COMMIT, 0, 0, 0), (ACTION, 0, 0, 0)], 3, flags, lanes, gangs=gangs, rows=rows, ops=ops, batch=True)
    got = c[4].q.reshape(-1, 6)
    assert got[:, 5].tolist() == list(range(len(got))) and [tuple(r[:3]) for r in got[:5].tolist()] == [o[:3] for o in under]


def test_a_pod_that_is_not_pending_refuses_the_call():
    """KAI_ERR_STATE with first_bad = the index in tasks, decided by the first launch: nothing is written, the Statement stays open"""
    snap, cfg, pend = binpack_scene(48)
    running = int(np.nonzero(snap.arrays["pod_status"] == S["Running"])[0][0])
    for flags in (0, EP):
        a, _, _ = place_script(snap, cfg, [(BEGIN, 0, 0, 0), (PLACE, flags, 0, 2), (PLACE, flags, 0, 1)], gangs=[(pend[:3], [-1]), ([pend[3], running, pend[4]], [-1])])
        assert (a[1].status, a[1].first_bad, a[1].log_len) == (-6, 4, 0)
        TS.same_all(a[1], a[0], "a refused call writes nothing")
        assert a[2].status == -6, "the prep kernel looks at every task of the call's list"


# ---- (9) a whole action composed
def action_scene():
    """one leaf queue; two racks of two 4-GPU nodes under one zone, rack B's first node half used.  Jobs in priority order: a gang of three 2-GPU tasks that requires a rack; a
    gang of two 3-GPU tasks that requires a rack; a gang of five 4-GPU tasks that requires the zone and fits nowhere (no node sets); a job without a constraint; a gang of two
    1-GPU tasks that prefers a rack, for which one GPU is left by then (its sets of the entry state are tried and rolled back).  Every job needs all of its tasks, so the action places a job whole or not at all."""
    import test_oracle_topology_kat as KAT
    rn = lambda rack: {"CPUMillis": 64000, "GPUs": 4, "MaxTaskNum": 100, "Labels": {"zone": "zone1", "rack": rack}}
    nodes = {"a1": rn("rackA"), "a2": rn("rackA"), "b1": rn("rackB"), "b2": rn("rackB")}
    gang = lambda name, prio, g, n, root: {"Name": name, "Priority": prio, "QueueName": "q", "RequiredGPUsPerTask": g, "RequiredCPUsPerTask": 1, "RootSubGroupSet": root, "Tasks": [{"State": "Pending"}] * n}
    jobs = [gang("three-twos", 90, 2, 3, KAT._root("rack")), gang("two-threes", 80, 3, 2, KAT._root("rack")), gang("too-large", 70, 4, 5, KAT._root("zone")),
            {"Name": "plain", "Priority": 60, "QueueName": "q", "RequiredGPUsPerTask": 1, "Tasks": [{"State": "Pending"}]}, gang("two-ones", 50, 1, 2, KAT._root("zone", "rack")),
            {"Name": "runs", "Priority": 50, "QueueName": "q", "RequiredGPUsPerTask": 2, "Tasks": [{"State": "Running", "NodeName": "b1"}]}]
    case = {"Name": "action", "Nodes": nodes, "Topologies": KAT.TOPO, "Queues": [{"Name": "q", "DeservedGPUs": 16}], "Jobs": jobs, "JobExpectedResults": {}}
    snap, cfg, _ = T.case_to_snapshot(case)
    cfg.plugins |= abi.PLUGINS["topology"]
    return snap, cfg


def oracle_job_sequence(ref):
    seq = []
    for o in ref.ops:
        if o[3] not in seq: seq.append(o[3])
    return seq


def pending_pods(snap, job):
    a = snap.arrays
    return [int(p) for p in np.nonzero((a["pod_job"] == job) & (a["pod_status"] == S["Pending"]))[0]]


@pytest.mark.parametrize("flags,lanes", MODES, ids=MODE_IDS)
def test_a_whole_allocate_action_in_one_call(flags, lanes):
    """every job of the scene in the oracle's pop order (the device's kai_job_order is compared with it in tests/test_gpu_stmt_place.py), its node sets and score row from one
    scored subset call at the entry state, ONE kai_stmt_place over all of them, commit: the oracle's operations and final state"""
    snap, cfg = action_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    order = [snap.job_names.index(n) for n in ("three-twos", "two-threes", "too-large", "plain", "two-ones")]
    assert oracle_job_sequence(ref) == order[:2] + order[3:4], "the oracle places the first two gangs and the plain job; the last gang finds one GPU left"
    with TSC.Sim(snap, cfg) as sim:
        r = sim.subset(order)
    assert r.call_status == 0
    gangs = [(pending_pods(snap, j), list(range(int(r.ans["first"][i]), int(r.ans["first"][i] + r.ans["n_sets"][i]))), i) for i, j in enumerate(order) if r.ans["status"][i] == 0 and r.ans["n_sets"][i] > 0]
    assert len(gangs) == 4 and r.ans["status"][2] == abi.SUBSET_NO_FIT, "no domain can take the five 4-GPU tasks: the caller has no sets to offer"
    data = dict(gangs=gangs, rows=list(r.masks), score_rows=r.score_rows, deciles=r.deciles)
    a, _ = against_the_loop(snap, cfg, [(BEGIN, 0, 0, 0)], [(COMMIT, 0, 0, 0)], len(gangs), flags, lanes, **data)
    assert [x[0] for x in a[1].answers] == [PLACED, PLACED, PLACED, NO_FIT] and a[1].answers[3][2] == 3, "the last gang's three sets (of the entry state) are tried and rolled back"
    assert [x[:4] for x in a[1].placed] == ref.ops, "the (kind, pod, node, job) sequence is the oracle's allocate"
    OA.same_state(a[2], ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "the composed action against the oracle")
