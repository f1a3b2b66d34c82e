"""kai_ops_apply without a GPU.

 - the export, the ABI struct and the flag values;
 - arguments and call order under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp, as tests/test_best_nodes.py does):
   every host-decidable refusal is made before the first device call, leaves `result` as specified, the device memory image and the session as they were; n_ops == 0
   makes no device call; a warm call makes one upload and two launches and allocates nothing: neither the number nor the bytes of the live device allocations change
   (a free followed by a larger allocation would change the bytes) and no pinned memory is taken.  The stand-in runtime counts no device-to-host copies and no
   synchronisations, so "one download, one synchronise" is asserted nowhere here: it is what oa_drive's read_head does, once per call on the chip-wide path;
 - the kernel bodies and the call's control flow (kai_ops_apply.hpp) run with emulated lanes by tests/host_sim/ops_apply_sim.cpp on a session of the host simulation,
   against the oracle: its Statement scripts and its whole actions, on both paths, with workgroups of 256, 100 and 1 lanes and with the wave order reversed.
The parity claim on the device is tests/test_gpu_ops_apply.py."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
S = abi.POD_STATUS
ALLOCATE, PIPELINE, EVICT = 0, 1, 2  # kai_op_kind
WIDE, ENGINE = abi.APPLY_PATH_WIDE, abi.APPLY_PATH_ENGINE
CYCLE = ("allocate", "consolidation", "reclaim", "preempt")
OP_DT = np.dtype([("seq", "<i8"), ("kind", "<i4"), ("pod", "<i4"), ("node", "<i4"), ("job", "<i4"), ("stmt", "<i4"), ("pad", "<i4")])


def test_exports_and_struct_sizes():
    assert "kai_ops_apply" in T.pkg.core.EXPORTS
    R = abi.KaiApplyResult
    assert C.sizeof(R) == 16 and [f[0] for f in R._fields_] == ["first_bad", "path", "statements"]
    assert R.first_bad.offset == 0 and R.path.offset == 8 and R.statements.offset == 12
    assert (abi.APPLY_CHECK_ONLY, abi.APPLY_ENGINE_PATH) == (1, 2) and (abi.APPLY_PATH_NONE, abi.APPLY_PATH_WIDE, abi.APPLY_PATH_ENGINE) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    for text in ("int kai_ops_apply(", "#define KAI_APPLY_CHECK_ONLY  0x1u", "#define KAI_APPLY_ENGINE_PATH 0x2u", "#define KAI_APPLY_PATH_WIDE 1", "#define KAI_APPLY_PATH_ENGINE 2",
                 "typedef struct kai_apply_result { int64_t first_bad; int32_t path; int32_t statements; } kai_apply_result;"):
        assert text in hdr, text
    assert hasattr(T.pkg.load_library(), "kai_ops_apply")
    assert hasattr(T.pkg.core.Session, "apply_ops")


# ---------------------------------------------------------------------------------------------- the host side under the host-only library
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
Op, Res = abi.KaiOp, abi.KaiApplyResult
lib.kai_ops_apply.argtypes = [C.c_void_p, C.POINTER(Op), C.c_int64, C.c_uint32, C.POINTER(Res)]
snap, cfg, _ = pkg.synth.config(1, 0.3)
P, N = snap.n_pods, snap.n_nodes
pending = [int(p) for p in np.nonzero(snap.arrays["pod_status"] == abi.POD_STATUS["Pending"])[0][:8]]
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def call(h, ops, n=None, flags=0, null=False, res=True):
    """ops: (kind, pod, node, stmt, pad) tuples.  Returns [status, first_bad, path, statements]."""
    arr = (Op * max(len(ops), 1))(*[Op(77, k, p, nd, -5, st, pad) for k, p, nd, st, pad in ops])
    r = Res(123, 45, 67)
    rc = lib.kai_ops_apply(h, None if null else arr, len(ops) if n is None else n, flags, C.byref(r) if res else None)
    return [rc, r.first_bad, r.path, r.statements]
good = [(0, pending[0], 0, 0, 0), (0, pending[1], 1, 0, 0), (0, pending[2], N - 1, 1, 0), (0, pending[3], 2, 3, 0)]
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
res["before_open"] = call(h, good)
res["empty_before_open"] = call(h, [])
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = image()
bad = {}
bad["null_ops"] = call(h, good, null=True)
bad["negative_count"] = call(h, good, n=-1)
bad["unknown_flags"] = call(h, good, flags=4)
bad["unknown_flags_high"] = call(h, good, flags=0x80000001)
bad["kind_3"] = call(h, good[:2] + [(3, pending[4], 0, 0, 0)] + good[2:])
bad["kind_negative"] = call(h, good[:2] + [(-1, pending[4], 0, 0, 0)] + good[2:])
bad["pod_negative"] = call(h, good[:2] + [(0, -1, 0, 0, 0)] + good[2:])
bad["pod_too_large"] = call(h, good[:2] + [(0, P, 0, 0, 0)] + good[2:])
bad["node_negative"] = call(h, good[:2] + [(0, pending[4], -1, 0, 0)] + good[2:])
bad["node_too_large"] = call(h, good[:2] + [(2, pending[4], N, 0, 0)] + good[2:])
bad["pad"] = call(h, good[:2] + [(0, pending[4], 0, 0, 9)] + good[2:])
bad["stmt_decreases"] = call(h, good[:3] + [(0, pending[4], 0, 0, 0)])
res["bad"] = bad
res["null_result"] = lib.kai_ops_apply(h, None, 3, 0, None)
res["image_unchanged"] = image() == img0
res["empty"] = call(h, []); res["empty_null"] = call(h, [], null=True)
res["image_unchanged_by_empty"] = image() == img0
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
res["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
# good calls: what each costs on the device (the kernels of the host-only library do nothing: the verdict that comes back is the one that was sent, "valid, every pod once")
res["good1"] = call(h, good); i1 = image()
res["good2"] = call(h, good); i2 = image()
res["good3"] = call(h, good[:2], res=False)[0]; i3 = image()
res["check_only"] = call(h, good, flags=1); i4 = image()
res["first_call"] = dict(allocations=i1[1] - img0[1], launches=i1[3] - img0[3], h2d=i1[4] - img0[4], memsets=i1[7] - img0[7], pinned=i1[8] - img0[8])
res["warm_call"] = dict(allocations=i2[1] - i1[1], live_bytes=i2[2] - i1[2], launches=i2[3] - i1[3], h2d=i2[4] - i1[4], h2d_bytes=i2[5] - i1[5], d2d=i2[6] - i1[6], memsets=i2[7] - i1[7], pinned=i2[8] - i1[8])
res["smaller_call"] = dict(allocations=i3[1] - i2[1], live_bytes=i3[2] - i2[2], launches=i3[3] - i2[3], h2d=i3[4] - i2[4])
res["check_only_call"] = dict(allocations=i4[1] - i3[1], live_bytes=i4[2] - i3[2], launches=i4[3] - i3[3], h2d=i4[4] - i3[4])
res["still_open_after"] = lib.kai_pod_states(h, st_out, nd_out, P)
lib.kai_core_destroy(h)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["sharded"] = call(h2, good)
lib.kai_core_destroy(h2)
# a session with shared-GPU requests
snap3, cfg3, _ = pkg.synth.config(1, 0.2); pkg.synth.add_fractions(snap3, 7, frac=0.3)
h3 = C.c_void_p(); st3 = snap3.as_struct()
assert lib.kai_core_create(C.byref(cfg3), 1, None, C.byref(h3)) == 0 and lib.kai_session_open(h3, C.byref(st3)) == 0
img3 = image()
res["shared"] = call(h3, [(0, 0, 0, 0, 0)]); res["shared_image_unchanged"] = image() == img3
lib.kai_core_destroy(h3)
print(json.dumps(res))
'''


def test_arguments_and_call_order(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["before_open"] == [-6, -1, 0, 0], "KAI_ERR_STATE without an open session"
    assert out["empty_before_open"][0] == -6
    no_single_op = ("null_ops", "negative_count", "unknown_flags", "unknown_flags_high")
    for k, (rc, first_bad, path, statements) in out["bad"].items():
        assert rc == -1, (k, rc)
        assert (path, statements) == (0, 0), k
        assert first_bad == (-1 if k in no_single_op else 3 if k == "stmt_decreases" else 2), (k, first_bad)
    assert out["null_result"] == -1, "result may be NULL"
    assert out["image_unchanged"], "a refused call allocated or wrote device memory"
    assert out["empty"] == [0, -1, 0, 0] and out["empty_null"] == [0, -1, 0, 0] and out["image_unchanged_by_empty"], "n_ops == 0: KAI_OK without a device call"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["sharded"] == [-5, -1, 0, 0], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["shared"] == [-5, -1, 0, 0] and out["shared_image_unchanged"], "KAI_ERR_UNSUPPORTED in a session with shared-GPU requests, before the first device call"
    assert out["good1"] == [0, -1, 1, 3] and out["good2"] == [0, -1, 1, 3] and out["good3"] == 0 and out["still_open_after"] == 0
    assert out["check_only"] == [0, -1, 1, 3]
    # the device side of a call: one upload, the check and the apply launch, one download; the first call of a handle also allocates its scratch (zeroed once) and its staging
    assert out["first_call"] == dict(allocations=1, launches=2, h2d=1, memsets=1, pinned=out["first_call"]["pinned"]) and out["first_call"]["pinned"] > 0
    w = out["warm_call"]
    assert w == dict(allocations=0, live_bytes=0, launches=2, h2d=1, h2d_bytes=64 + 4 * 32, d2d=0, memsets=0, pinned=0), w
    assert out["smaller_call"] == dict(allocations=0, live_bytes=0, launches=2, h2d=1)
    assert out["check_only_call"] == dict(allocations=0, live_bytes=0, launches=2, h2d=1)


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "ops_apply_sim.cpp")


def sim_lib():
    so = os.path.join(ROOT, "tests", "host_sim", "libopsapplysim.so")
    deps = [SIM_SRC, os.path.join(ROOT, "tests", "host_sim", "sim_session.hpp"), os.path.join(ROOT, "tests", "host_sim", "native_bucket_fill.hpp")] + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_oasim_run.restype = C.c_int
    return lib


def make_ops(rows, stmts=None):
    """rows: (kind, pod, node[, job]) tuples -> a kai_op array; stmts: the Statement ids (default: one Statement)."""
    a = np.zeros(len(rows), OP_DT)
    for i, r in enumerate(rows):
        a[i]["kind"], a[i]["pod"], a[i]["node"] = r[0], r[1], r[2]
        a[i]["job"] = r[3] if len(r) > 3 else -1
        a[i]["seq"] = i
    a["stmt"] = 0 if stmts is None else np.asarray(stmts, np.int32)
    return a


def sim_run(snap, cfg, batch, pre=(), post=(), flags=0, lanes=256, calls=None, no_batch=False):
    """no_batch: the cycle's own allocate actions run on the sequential engine (KAI_HOSTSIM_NO_BATCH: the emulated batch path takes minutes from a few thousand pods on).
    -> Result: apply_status, result (first_bad, path, statements), paths, mid (state right behind the apply: pod_status, pod_node, nodes, shares, hidden), and the
    cycle's operations / final state as T.Oracle.run returns them.  calls: the batch as consecutive calls [(lo, hi), ...]."""
    lib = sim_lib()
    s = snap.as_struct()
    P, Q, N = snap.n_pods, snap.n_queues, snap.n_nodes
    ai = lambda names: (C.c_int * max(len(names), 1))(*[abi.ACTIONS[a] for a in names])
    batch = np.ascontiguousarray(batch, dtype=OP_DT)
    off = None if calls is None else np.ascontiguousarray([c[0] for c in calls] + [calls[-1][1]], dtype=np.int64)
    n_calls = 1 if calls is None else len(calls)
    paths = np.full(n_calls, -1, np.int32)
    cap = max(64, 8 * P)
    ops = (abi.KaiOp * cap)(); n_ops = C.c_int64(0)
    status = np.zeros(P, np.int32); node = np.zeros(P, np.int32); mstatus = np.zeros(P, np.int32); mnode = np.zeros(P, np.int32)
    sh_mid = (abi.KaiQueueShare * max(Q, 1))(); sh_fin = (abi.KaiQueueShare * max(Q, 1))(); nd_mid = (abi.KaiNodeState * max(N, 1))(); nd_fin = (abi.KaiNodeState * max(N, 1))()
    hidden = np.zeros(4 * P + 4 * snap.n_podsets + 8 * snap.n_jobs + 8, np.int32); n_hidden = C.c_int64(0)
    rc_apply = C.c_int(99); res = abi.KaiApplyResult()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    had = os.environ.get("KAI_HOSTSIM_NO_BATCH")
    if no_batch: os.environ["KAI_HOSTSIM_NO_BATCH"] = "1"
    try:
        rc = lib.kai_oasim_run(C.byref(cfg), C.byref(s), ai(pre), len(pre), batch.ctypes.data_as(C.POINTER(abi.KaiOp)), C.c_int64(len(batch)), C.c_uint32(flags), C.c_int(lanes),
                               None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(n_calls), ip(paths), ai(post), len(post), C.byref(rc_apply), C.byref(res),
                               ip(mstatus), ip(mnode), sh_mid, nd_mid, ip(hidden), C.c_int64(len(hidden)), C.byref(n_hidden),
                               ops, C.c_int64(cap), C.byref(n_ops), ip(status), ip(node), sh_fin, nd_fin)
    finally:
        if no_batch and had is None: del os.environ["KAI_HOSTSIM_NO_BATCH"]
    assert rc == 0, f"kai_oasim_run rc={rc}"
    mid = T.Result(pod_status=mstatus, pod_node=mnode, shares=T.shares_to_np(sh_mid, Q), nodes=T.nodes_to_np(nd_mid, N, snap.n_res), hidden=hidden[: n_hidden.value].copy())
    return T.Result(apply_status=rc_apply.value, first_bad=res.first_bad, path=res.path, statements=res.statements, paths=paths.tolist(), mid=mid,
                    ops=[(o.kind, o.pod, o.node, o.job) for o in ops[: n_ops.value]], stmts=[o.stmt for o in ops[: n_ops.value]], pod_status=status, pod_node=node,
                    shares_final=T.shares_to_np(sh_fin, Q), nodes=T.nodes_to_np(nd_fin, N, snap.n_res))


def same_state(got, ref_status, ref_node, ref_nodes, ref_shares=None, what=""):
    assert (got.pod_status == ref_status).all(), f"{what}: pod status, pods {np.nonzero(got.pod_status != ref_status)[0][:8].tolist()}"
    assert (got.pod_node == ref_node).all(), f"{what}: pod node"
    for k in ref_nodes:
        assert np.array_equal(got.nodes[k], ref_nodes[k]), f"{what}: node {k}"
    if ref_shares is not None:
        shares = got.shares if hasattr(got, "shares") else got.shares_final
        for k in ref_shares:
            assert np.array_equal(shares[k], ref_shares[k]), f"{what}: share {k}"


def same_mid(a, b, what=""):
    same_state(a.mid, b.mid.pod_status, b.mid.pod_node, b.mid.nodes, b.mid.shares, what)
    assert np.array_equal(a.mid.hidden, b.mid.hidden), f"{what}: the state no read-back shows differs at words {np.nonzero(a.mid.hidden != b.mid.hidden)[0][:8].tolist()}"


# ---- (a) the oracle's Statement scripts
O_EVICT, O_ALLOCATE, O_PIPELINE = 1, 2, 3  # operation codes of kai_oracle_statement_script (tests/test_oracle_statement.py)
TO_ORACLE = {ALLOCATE: O_ALLOCATE, PIPELINE: O_PIPELINE, EVICT: O_EVICT}


def script_sessions():
    import test_oracle_statement as tos
    snap, cfg = tos.session()
    run, pend = snap.pod_names.index(tos.RUN), snap.pod_names.index(tos.PEND)
    yield "two_tasks", snap, cfg, [[(EVICT, run, 0)], [(ALLOCATE, pend, 0)], [(PIPELINE, pend, 0)], [(EVICT, run, 0), (ALLOCATE, pend, 0)], [(EVICT, run, 0), (PIPELINE, run, 0)],
                                   [(ALLOCATE, pend, 0), (EVICT, pend, 0)], [(PIPELINE, pend, 0), (EVICT, pend, 0)], [(EVICT, run, 0), (EVICT, run, 0)], [(EVICT, run, 0), (PIPELINE, pend, 0)]]
    case = {"Name": "statement", "Nodes": {"node0": {"GPUs": 2}}, "Queues": [{"Name": "queue0", "DeservedGPUs": 2}],
            "Jobs": [{"Name": "pending_job0", "RequiredGPUsPerTask": 1, "QueueName": "queue0", "Priority": 50, "Tasks": [{"State": "Pending"}]},
                     {"Name": "running_job0", "RequiredGPUsPerTask": 1, "QueueName": "queue0", "Priority": 50, "Tasks": [{"State": "Running", "NodeName": "node0"}] * 2}], "JobExpectedResults": {}}
    snap, cfg, _ = T.case_to_snapshot(case); cfg.plugins = 0
    pend = snap.pod_names.index(tos.PEND); r0, r1 = [i for i in range(snap.n_pods) if i != pend]
    yield "full_node", snap, cfg, [[(PIPELINE, pend, 0)], [(EVICT, r0, 0), (EVICT, r1, 0), (PIPELINE, pend, 0)], [(EVICT, r0, 0), (PIPELINE, r0, 0), (EVICT, r1, 0)]]
    snap, cfg, _ = T.pkg.synth.config(0)
    cfg = abi.copy_config(cfg); cfg.plugins = 0  # as the two sessions above: the oracle's script runs a Statement on a session without plugins
    st, nd = snap.arrays["pod_status"], snap.arrays["pod_node"]
    pending = np.nonzero(st == S["Pending"])[0]; placed = np.nonzero((st == S["Running"]) & (nd >= 0))[0]
    N = snap.n_nodes
    alloc = [(ALLOCATE, int(p), int(i % N)) for i, p in enumerate(pending[:20])]
    pipe = [(PIPELINE, int(p), int((3 * i + 1) % N)) for i, p in enumerate(pending[20:30])]
    evict = [(EVICT, int(p), int(nd[p])) for p in placed[:10]]
    again = [(PIPELINE, int(p), int((nd[p] + 1) % N)) for p in placed[:4]] + [(EVICT, int(pending[0]), 0)]
    yield "config0", snap, cfg, [alloc, alloc + pipe + evict, evict + alloc[:5] + again]


SCRIPTS = [(name, i) for name, _, _, scripts in script_sessions() for i in range(len(scripts))]


@pytest.fixture(scope="module")
def script_cases():
    out = {}
    import test_oracle_statement as tos
    for name, snap, cfg, scripts in script_sessions():
        for i, sc in enumerate(scripts):
            res, st, nd, nodes = tos.run_script(snap, cfg, [(TO_ORACLE[k], p, n, 1) for k, p, n in sc])
            assert all(res), (name, i, res)  # every operation of these scripts is legal
            st = np.array(st, np.int32)
            for k, p, _ in sc:  # the script stops before the commit, which calls BindPod for every Allocate operation of the Statement, whatever came behind it (statement.go:536-575, session.go:111-126)
                if k == ALLOCATE: st[p] = S["Binding"]
            out[name, i] = (snap, cfg, sc, st, np.array(nd, np.int32), nodes)
    return out


@pytest.mark.parametrize("name,i", SCRIPTS, ids=[f"{n}-{i}" for n, i in SCRIPTS])
def test_statement_scripts_against_the_oracle(script_cases, name, i):
    """allocate / pipeline / evict scripts: pod status and node, node Idle / Releasing / Used as the oracle's Statement leaves them; the two paths agree in everything"""
    snap, cfg, sc, st, nd, nodes = script_cases[name, i]
    named_twice = len({p for _, p, _ in sc}) < len(sc)
    got = {}
    for flags in (0, abi.APPLY_ENGINE_PATH):
        for lanes in (256, 100, 1):
            r = sim_run(snap, cfg, make_ops(sc), flags=flags, lanes=lanes)
            assert r.apply_status == 0 and r.first_bad == -1 and r.statements == 1, (r.apply_status, r.first_bad)
            if flags or named_twice: assert r.path == ENGINE
            same_state(r.mid, st, nd, nodes, what=f"flags {flags} lanes {lanes}")
            got[flags, lanes] = r
    for k in got: same_mid(got[k], got[0, 256], str(k))


# ---- (b) whole actions of the oracle
def per_action(snap, cfg, actions):
    """the oracle's run of `actions`, and its operations cut into the actions they belong to (the run of a prefix of the actions is a prefix of the run)"""
    full = T.Oracle.run(snap, cfg, actions)
    cuts = [0] + [len(T.Oracle.run(snap, cfg, actions[:k]).ops) for k in range(1, len(actions))] + [len(full.ops)]
    return full, cuts


def ref_ops(ref, lo=0, hi=None):
    hi = len(ref.ops) if hi is None else hi
    return make_ops(ref.ops[lo:hi], ref.stmts[lo:hi])


def statement_prefix(stmts, want):
    """the cut between two Statements that is nearest to `want` operations"""
    cuts = [i for i in range(1, len(stmts) + 1) if i == len(stmts) or stmts[i] != stmts[i - 1]]
    return min(cuts, key=lambda c: (abs(c - want), c))


@pytest.fixture(scope="module")
def allocate_case():
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    return snap, cfg, T.Oracle.run(snap, cfg, ("allocate",))


def test_allocate_batch_on_the_wide_path(allocate_case):
    snap, cfg, ref = allocate_case
    assert (snap.n_nodes, snap.n_pods, len(ref.ops), len(set(ref.stmts))) == (300, 3277, 649, 196)
    assert max(np.bincount([o[2] for o in ref.ops])) <= 6
    first = None
    for lanes in (256, 100, 1):
        r = sim_run(snap, cfg, ref_ops(ref), lanes=lanes)
        assert (r.apply_status, r.first_bad, r.path, r.statements) == (0, -1, WIDE, 196)
        same_state(r.mid, ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, f"the whole action, {lanes} lanes")
        e = sim_run(snap, cfg, ref_ops(ref), flags=abi.APPLY_ENGINE_PATH, lanes=lanes)
        assert (e.apply_status, e.path, e.statements) == (0, ENGINE, 196)
        same_state(e.mid, ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, f"the whole action on the engine path, {lanes} lanes")
        first = first or r
        same_mid(r, first, f"{lanes} lanes against 256"); same_mid(e, first, f"engine against wide, {lanes} lanes")
    # the allocate action behind it finds what the oracle's own second allocate finds
    ref2 = T.Oracle.run(snap, cfg, ("allocate", "allocate"))
    again = sim_run(snap, cfg, ref_ops(ref), post=("allocate",), no_batch=True)
    assert again.ops == ref2.ops[len(ref.ops):]
    same_state(again, ref2.pod_status, ref2.pod_node, ref2.nodes, ref2.shares_final, "allocate behind the apply")


@pytest.mark.parametrize("lanes", [256, 100, 1])
@pytest.mark.parametrize("want", [1, 63, 64, 65, 257])
def test_allocate_prefixes_on_both_paths(allocate_case, want, lanes):
    """prefixes of whole Statements: the chip-wide path against the engine walk, in everything they leave and in the allocate action run behind either"""
    snap, cfg, ref = allocate_case
    n = statement_prefix(ref.stmts, want)
    post = ("allocate",) if lanes == 256 else ()
    w = sim_run(snap, cfg, ref_ops(ref, 0, n), lanes=lanes, post=post, no_batch=True)
    e = sim_run(snap, cfg, ref_ops(ref, 0, n), lanes=lanes, flags=abi.APPLY_ENGINE_PATH, post=post, no_batch=True)
    assert (w.apply_status, w.path, e.apply_status, e.path) == (0, WIDE, 0, ENGINE) and w.statements == e.statements == len(set(ref.stmts[:n]))
    same_mid(w, e, f"prefix of {n}")
    if post:  # an allocate action behind either: the same operations, the same end (the oracle's own action, going on behind the prefix, pops jobs off heaps keyed before it: no reference for a fresh action)
        assert w.ops == e.ops and len(w.ops) > 0
        same_state(w, e.pod_status, e.pod_node, e.nodes, e.shares_final, f"allocate behind a prefix of {n}")


@pytest.fixture(scope="module")
def crowded_cases():
    return {seed: (crowded(seed),) + per_action(*crowded(seed), CYCLE) for seed in range(12)}


def named_twice(ops):
    pods = [o[1] for o in ops]
    return len(set(pods)) < len(pods)


@pytest.mark.parametrize("flags,lanes", [(0, 256), (0, 100), (0, 1), (abi.APPLY_ENGINE_PATH, 256), (abi.APPLY_ENGINE_PATH, 100), (abi.APPLY_ENGINE_PATH, 1)],
                         ids=["wide256", "wide100", "wide1", "engine256", "engine100", "engine1"])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("seed", range(12))
def test_the_cycle_goes_on(crowded_cases, seed, k, flags, lanes):
    """the oracle's operations of the first k actions applied, one call per action; the remaining actions run by the engine: the whole cycle as the oracle ran it.
    flags 0: every call takes the path it qualifies for; KAI_APPLY_ENGINE_PATH: the engine walk also where the chip-wide path would do."""
    (snap, cfg), ref, cuts = crowded_cases[seed]
    calls = [(cuts[i], cuts[i + 1]) for i in range(k)]
    r = sim_run(snap, cfg, ref_ops(ref, 0, cuts[k]), post=CYCLE[k:], calls=calls, flags=flags, lanes=lanes)
    assert r.apply_status == 0, (r.apply_status, r.first_bad)
    for i, (lo, hi) in enumerate(calls):  # which path took each call: a pod named twice, or a start state the chip-wide path leaves to the engine
        if hi == lo: assert r.paths[i] == abi.APPLY_PATH_NONE
        elif flags or named_twice(ref.ops[lo:hi]): assert r.paths[i] == ENGINE, (i, r.paths)
        else: assert r.paths[i] in (WIDE, ENGINE)
    assert r.ops == ref.ops[cuts[k]:]
    base = ref.stmts[cuts[k] - 1] + 1 if cuts[k] else 0  # (the host simulation numbers the Statements of one cycle from 0; the applied ones are not its own)
    assert [s + base for s in r.stmts] == ref.stmts[cuts[k]:]
    same_state(r, ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, f"seed {seed} k {k}")


def test_the_cycle_takes_the_wide_path_somewhere(crowded_cases):
    """(so that "WIDE or ENGINE" above is not "always ENGINE") some of the applied actions are taken chip-wide (not every seed has one: an action may commit nothing,
    or name a pod twice)"""
    wide = 0
    for seed in range(12):
        (snap, cfg), ref, cuts = crowded_cases[seed]
        r = sim_run(snap, cfg, ref_ops(ref, 0, cuts[3]), post=CYCLE[3:], calls=[(cuts[i], cuts[i + 1]) for i in range(3)])
        wide += r.paths.count(WIDE)
    assert wide >= 1, wide


WIDE_VICTIM = [(0, "reclaim", (2, 2)), (6, "reclaim", (1, 5)), (11, "preempt", (3, 2))]


@pytest.mark.parametrize("lanes", [256, 100, 1])
@pytest.mark.parametrize("seed,action,counts", WIDE_VICTIM, ids=[f"crowded{s}-{a}" for s, a, _ in WIDE_VICTIM])
def test_evictions_and_pipelines_on_the_wide_path(seed, action, counts, lanes):
    snap, cfg = crowded(seed)
    ref = T.Oracle.run(snap, cfg, (action,))
    kinds = [o[0] for o in ref.ops]
    assert (kinds.count(EVICT), kinds.count(PIPELINE)) == counts and not named_twice(ref.ops)
    w = sim_run(snap, cfg, ref_ops(ref), lanes=lanes)
    e = sim_run(snap, cfg, ref_ops(ref), lanes=lanes, flags=abi.APPLY_ENGINE_PATH)
    assert (w.apply_status, w.path, e.apply_status, e.path) == (0, WIDE, 0, ENGINE)
    same_state(w.mid, ref.pod_status, ref.pod_node, ref.nodes, ref.shares_final, "wide")
    same_mid(w, e, "wide against engine")


def refusal_cases(snap, ref):
    """(name, batch, index of the offending operation): one per precondition, the offender in the middle of the oracle's valid allocate batch"""
    st, nd = snap.arrays["pod_status"], snap.arrays["pod_node"]
    used = {o[1] for o in ref.ops}
    running = [int(p) for p in np.nonzero((st == S["Running"]) & (nd >= 0))[0] if p not in used]
    pending = [int(p) for p in np.nonzero(st == S["Pending"])[0] if p not in used]
    mid = len(ref.ops) // 2
    def with_op(row):
        rows = list(ref.ops[:mid]) + [row] + list(ref.ops[mid:]); stmts = ref.stmts[:mid] + [ref.stmts[mid - 1]] + ref.stmts[mid:]
        return make_ops(rows, stmts)
    other = (int(nd[running[0]]) + 1) % snap.n_nodes
    yield "allocate_a_running_pod", with_op((ALLOCATE, running[0], 0)), mid
    yield "pipeline_a_running_pod", with_op((PIPELINE, running[0], 0)), mid
    yield "evict_a_pending_pod", with_op((EVICT, pending[0], 0)), mid
    yield "evict_from_another_node", with_op((EVICT, running[0], other)), mid
    yield "allocate_twice", with_op((ALLOCATE, ref.ops[0][1], ref.ops[0][2])), mid  # (a pod named twice: the engine walk's shadow finds it)
    p, n = ref.ops[mid + 1][1], ref.ops[mid + 1][2]
    yield "evict_before_its_allocate", with_op((EVICT, p, n)), mid


def test_refusals_write_nothing():
    snap, cfg = crowded(4)
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    assert len(ref.ops) >= 4
    untouched = sim_run(snap, cfg, make_ops([]), post=("reclaim",))
    for name, batch, bad in refusal_cases(snap, ref):
        for flags in (0, abi.APPLY_ENGINE_PATH, abi.APPLY_CHECK_ONLY):
            r = sim_run(snap, cfg, batch, post=("reclaim",), flags=flags)
            assert (r.apply_status, r.first_bad, r.path, r.statements) == (-6, bad, 0, 0), (name, flags, r.apply_status, r.first_bad)
            same_mid(r, untouched, name)
            assert r.ops == untouched.ops and r.stmts == untouched.stmts, name
            same_state(r, untouched.pod_status, untouched.pod_node, untouched.nodes, untouched.shares_final, name)
    # check only: a valid batch is reported valid and writes nothing
    r = sim_run(snap, cfg, ref_ops(ref), post=("reclaim",), flags=abi.APPLY_CHECK_ONLY)
    assert (r.apply_status, r.first_bad, r.statements) == (0, -1, len(set(ref.stmts)))
    same_mid(r, untouched, "check only")
    assert r.ops == untouched.ops


REVERSED = r'''
import json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import test_ops_apply as t
out = {}
snap, cfg, _ = t.T.pkg.synth.config(1, 0.3); ref = t.T.Oracle.run(snap, cfg, ("allocate",))
r = t.sim_run(snap, cfg, t.ref_ops(ref))
out["allocate"] = [r.apply_status, r.path, t.T.state_sha256(t.T.Result(pod_status=r.mid.pod_status, pod_node=r.mid.pod_node, nodes=r.mid.nodes, shares_final=r.mid.shares)), t.T.state_sha256(ref)]
for seed, action, _ in t.WIDE_VICTIM:
    snap, cfg = t.crowded(seed); ref = t.T.Oracle.run(snap, cfg, (action,))
    r = t.sim_run(snap, cfg, t.ref_ops(ref))
    out[f"{seed}-{action}"] = [r.apply_status, r.path, t.T.state_sha256(t.T.Result(pod_status=r.mid.pod_status, pod_node=r.mid.pod_node, nodes=r.mid.nodes, shares_final=r.mid.shares)), t.T.state_sha256(ref)]
print(json.dumps(out))
'''


def test_kernel_bodies_with_the_wave_order_reversed():
    """the emulator's waves take their turns in reverse (KW_EMU_ORDER=1, read once per process: a fresh one): sums through LDS that leaned on the waves' order would differ"""
    sim_lib()  # built before the child starts
    env = dict(os.environ, KW_EMU_ORDER="1")
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + REVERSED], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == 4
    for k, (status, path, sha, want) in got.items():
        assert (status, path) == (0, WIDE) and sha == want, k


def test_stand_alone_program(tmp_path):
    """the fixed case behind -DKAI_OASIM_MAIN (the program the sanitizers are run on) builds and agrees with itself: wide path, engine path, 256 / 100 / 1 lanes"""
    exe = str(tmp_path / "ops_apply_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKAI_OASIM_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ops_apply_sim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
