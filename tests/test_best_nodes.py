"""kai_best_nodes without a GPU.

 - the export and the two ABI structs;
 - arguments and call order under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp, as tests/test_session_rows.py does):
   every refusal is decided before the first device call, leaves `out` and the session's device memory as they were and the session open; a warm handle makes
   one upload, three launches and no allocation per call;
 - the three kernel bodies (kai_best_nodes.hpp) run with emulated lanes by tests/host_sim/best_nodes_sim.cpp over arrays in name-rank order, against the oracle.
The parity claim on the device is tests/test_gpu_best_nodes.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi


def test_exports_and_struct_sizes():
    assert "kai_best_nodes" in T.pkg.core.EXPORTS
    assert C.sizeof(abi.KaiNodeQuery) == 16 and C.sizeof(abi.KaiNodeAnswer) == 8
    assert [f[0] for f in abi.KaiNodeQuery._fields_] == ["pod", "nodeset", "flags", "pad"]
    assert abi.KaiNodeQuery.nodeset.offset == 4 and abi.KaiNodeQuery.flags.offset == 8 and abi.KaiNodeAnswer.is_pipeline.offset == 4
    assert abi.QUERY_PIPELINE_ONLY == 1
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    assert "int kai_best_nodes(" in hdr and "#define KAI_QUERY_PIPELINE_ONLY 0x1u" in hdr
    assert hasattr(T.pkg.load_library(), "kai_best_nodes")


DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
Q, A = abi.KaiNodeQuery, abi.KaiNodeAnswer
lib.kai_best_nodes.argtypes = [C.c_void_p, C.POINTER(Q), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(A)]
snap, cfg, _ = pkg.synth.config(1, 0.3)
P, N = snap.n_pods, snap.n_nodes
W = (N + 31) // 32
SENT = 0x5a5a5a5a
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def call(h, qs, n=None, rows=2, bits=True, out=True):
    """qs: (pod, nodeset, flags, pad) tuples.  Returns (status, out untouched)."""
    arr = (Q * max(len(qs), 1))(*[Q(*q) for q in qs])
    words = (C.c_uint32 * max(rows * W, 1))(*([0xffffffff] * max(rows * W, 1)))
    o = (A * max(len(qs), 1))(*[A(SENT, SENT) for _ in range(max(len(qs), 1))])
    rc = lib.kai_best_nodes(h, arr, len(qs) if n is None else n, words if bits else None, rows, o if out else None)
    return rc, all(x.node == SENT and x.is_pipeline == SENT for x in o)
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
good = [(0, -1, 0, 0), (1, 0, 1, 0), (P - 1, 1, 0, 0), (1, 0, 1, 0)]
res["before_open"] = call(h, good)
res["empty_before_open"] = call(h, [])
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = image()
bad = {}
bad["null_queries"] = (lib.kai_best_nodes(h, None, 2, None, 0, (A * 2)()), True)
bad["null_out"] = call(h, good, out=False)
bad["null_bitmaps"] = call(h, good, bits=False)
bad["negative_queries"] = call(h, good, n=-1)
bad["negative_nodesets"] = call(h, [(0, -1, 0, 0)], rows=-1)
bad["pod_negative"] = call(h, good + [(-1, -1, 0, 0)])
bad["pod_too_large"] = call(h, good + [(P, -1, 0, 0)])
bad["nodeset_too_large"] = call(h, good + [(0, 2, 0, 0)])
bad["nodeset_below_minus_one"] = call(h, good + [(0, -2, 0, 0)])
bad["nodeset_without_rows"] = call(h, [(0, 0, 0, 0)], rows=0)
bad["unknown_flags"] = call(h, good + [(0, -1, 2, 0)])
bad["unknown_flags_high"] = call(h, [(0, -1, 0x80000001, 0)] + good)
bad["pad"] = call(h, good + [(0, -1, 0, 7)])
res["bad"] = bad
res["image_unchanged"] = image() == img0
res["empty"] = call(h, [])
res["empty_null_arrays"] = lib.kai_best_nodes(h, None, 0, None, 0, None)
res["image_unchanged_by_empty"] = image() == img0
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
res["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
# good calls: what each costs on the device (the kernels of the host-only library do nothing; the counters are fake_hip's)
res["good1"] = call(h, good)[0]; i1 = image()
res["good2"] = call(h, good)[0]; i2 = image()
res["good3"] = call(h, good[:2], rows=1)[0]; i3 = image()
res["first_call"] = dict(allocations=i1[1] - img0[1], launches=i1[3] - img0[3], h2d=i1[4] - img0[4], pinned=i1[8] - img0[8])
res["warm_call"] = dict(allocations=i2[1] - i1[1], launches=i2[3] - i1[3], h2d=i2[4] - i1[4], h2d_bytes=i2[5] - i1[5], d2d=i2[6] - i1[6], memsets=i2[7] - i1[7], pinned=i2[8] - i1[8])
res["smaller_call"] = dict(allocations=i3[1] - i2[1], launches=i3[3] - i2[3], h2d=i3[4] - i2[4])
res["first_h2d_bytes"] = i1[5] - img0[5]
res["N"] = N; res["W"] = W
res["still_open_after"] = lib.kai_pod_states(h, st_out, nd_out, P)
lib.kai_core_destroy(h)
# a handle of a sharded group
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["sharded"] = call(h2, good)
lib.kai_core_destroy(h2)
print(json.dumps(res))
'''


def test_arguments_and_call_order(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["before_open"] == [-6, True], "KAI_ERR_STATE without an open session, out untouched"
    assert out["empty_before_open"][0] == -6
    for k, (rc, untouched) in out["bad"].items():
        assert rc == -1, (k, rc)
        assert untouched, f"{k}: a refused call wrote to out"
    assert out["image_unchanged"], "a refused call allocated or wrote device memory"
    assert out["empty"] == [0, True] and out["empty_null_arrays"] == 0 and out["image_unchanged_by_empty"], "n_queries == 0: KAI_OK without a device call"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["sharded"] == [-5, True], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["good1"] == 0 and out["good2"] == 0 and out["good3"] == 0 and out["still_open_after"] == 0
    # the device side of a call: one upload, three launches (the default configuration bin-packs: the range kernel runs); the first call of a session also allocates the handle's
    # scratch and sends the permutation in the same upload
    assert out["first_call"]["launches"] == 3 and out["first_call"]["h2d"] == 1 and out["first_call"]["allocations"] == 1
    assert out["first_h2d_bytes"] >= 4 * out["N"] + 4 * 16 + 2 * 4 * out["W"]
    w = out["warm_call"]
    assert w == dict(allocations=0, launches=3, h2d=1, h2d_bytes=w["h2d_bytes"], d2d=0, memsets=0, pinned=0), w
    assert w["h2d_bytes"] < 4 * 16 + 2 * 4 * out["W"] + 6 * 4 + 64, "a warm call sends the queries, the rows and the zeroed range flags only"
    assert out["smaller_call"] == dict(allocations=0, launches=3, h2d=1)


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
class BnSimIn(C.Structure):
    _fields_ = [("N", C.c_int32), ("P", C.c_int32), ("R", C.c_int32), ("n_pod_classes", C.c_int32), ("n_node_classes", C.c_int32),
                ("plugins", C.c_uint32), ("gpu_strategy", C.c_int32), ("cpu_strategy", C.c_int32), ("restrict_nodes", C.c_int32), ("pad", C.c_int32),
                ("n_alloc", C.c_void_p), ("n_flags", C.c_void_p), ("n_gpu_count", C.c_void_p), ("n_class", C.c_void_p), ("n_idle", C.c_void_p), ("n_rel", C.c_void_p),
                ("p_req", C.c_void_p), ("p_class", C.c_void_p), ("p_nominated", C.c_void_p), ("p_job", C.c_void_p), ("class_fit", C.c_void_p), ("perm", C.c_void_p)]


SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "best_nodes_sim.cpp")


def sim_lib():
    import glob
    so = os.path.join(ROOT, "tests", "host_sim", "libbestnodessim.so")
    deps = [SIM_SRC] + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_bnsim_run.restype = C.c_int
    lib.kai_bnsim_run.argtypes = [C.POINTER(BnSimIn), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return lib


Q_DT = np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("pad", "<i4")])
A_DT = np.dtype([("node", "<i4"), ("is_pipeline", "<i4")])
PLUGINS_NO_PROPORTION = abi.PLUGIN_ALL & ~abi.PLUGIN_PROPORTION


def the_snapshot():
    """the snapshot of test_gpu_best_node_with_node_sets: 150 nodes whose name order differs from their index order, 400 pending pods"""
    return T.pkg.synth.make_snapshot(150, 400, 4242, queue_levels=(2, 2), prefill=0.5, gpu_mix=((8, .5), (4, .3), (0, .2)), cpu_only_frac=0.3, lexi_names=True)


def rows_and_queries(snap, seed=5):
    """rows of density 0, 0.02, 0.2, 0.7 and 1 (caller's node indices) and, for 64 pending pods, a query per row and one over all nodes; every third asks PIPELINE_ONLY"""
    rng = np.random.default_rng(seed)
    N = snap.n_nodes
    masks = [rng.random(N) < d for d in (0.0, 0.02, 0.2, 0.7)] + [np.ones(N, bool)]
    W = (N + 31) // 32
    words = np.zeros((len(masks), W), np.uint32)
    for s, m in enumerate(masks):
        idx = np.nonzero(m)[0]
        np.bitwise_or.at(words[s], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    pending = np.nonzero(snap.arrays["pod_status"] == abi.POD_STATUS["Pending"])[0]
    pods = rng.choice(pending, size=64, replace=False)
    q = np.zeros(len(pods) * (len(masks) + 1), Q_DT)
    q["pod"] = np.repeat(pods, len(masks) + 1)
    q["nodeset"] = np.tile(np.arange(-1, len(masks)), len(pods))
    q["flags"] = (np.arange(len(q)) % 3 == 0).astype(np.uint32)
    return words, q


def oracle_answers(snap, cfg, words, q):
    lib = T.Oracle.lib(); lib.kai_oracle_best_node.restype = C.c_int
    s = snap.as_struct()
    out = np.zeros(len(q), A_DT)
    for i, x in enumerate(q):
        row = None if x["nodeset"] < 0 else np.ascontiguousarray(words[x["nodeset"]]).ctypes.data_as(C.POINTER(C.c_uint32))
        node, pipe = C.c_int(-1), C.c_int(0)
        assert lib.kai_oracle_best_node(C.byref(cfg), C.byref(s), int(x["pod"]), row, int(x["flags"] & 1), C.byref(node), C.byref(pipe)) == 0
        out[i] = (node.value, pipe.value)
    return out


def sim_answers(snap, cfg, words, q, lanes=256, grid=1 << 20):
    """The session state a fresh open would hold, in numpy: nodes in name-rank order, Idle / Releasing from the snapshot's active and Releasing pods (node_info.go:457-493)."""
    a = snap.arrays
    N, P, R = snap.n_nodes, snap.n_pods, snap.n_res
    perm = np.argsort(a["node_name_rank"], kind="stable").astype(np.int32)  # name rank -> caller's index
    rank_of = np.empty(N, np.int32); rank_of[perm] = np.arange(N, dtype=np.int32)
    alloc = np.ascontiguousarray(a["node_allocatable"][:, perm])
    st, nd = a["pod_status"], a["pod_node"]
    idle, rel = alloc.copy(), np.zeros_like(alloc)
    releasing, pipelined = st == abi.POD_STATUS["Releasing"], st == abi.POD_STATUS["Pipelined"]
    taking = ((st & abi.ACTIVE_USED) != 0) & ~pipelined & (nd >= 0)
    for r in range(R):
        np.subtract.at(idle[r], rank_of[nd[taking]], a["pod_req"][r, taking])
        np.add.at(rel[r], rank_of[nd[releasing & (nd >= 0)]], a["pod_req"][r, releasing & (nd >= 0)])
        np.subtract.at(rel[r], rank_of[nd[pipelined & (nd >= 0)]], a["pod_req"][r, pipelined & (nd >= 0)])
    nom = a["pod_nominated_node"]
    keep = dict(alloc=alloc, flags=np.ascontiguousarray(a["node_flags"][perm]), gcount=np.ascontiguousarray(a["node_gpu_count"][perm]), ncls=np.ascontiguousarray(a["node_class"][perm]),
                idle=idle, rel=rel, req=np.ascontiguousarray(a["pod_req"]), pcls=a["pod_class"], pnom=np.where(nom >= 0, rank_of[np.maximum(nom, 0)], -1).astype(np.int32),
                pjob=a["pod_job"], fit=np.ascontiguousarray(a["class_fit"]), perm=perm)
    i = BnSimIn(N=N, P=P, R=R, n_pod_classes=snap.n_pod_classes, n_node_classes=snap.n_node_classes, plugins=cfg.plugins, gpu_strategy=cfg.gpu_strategy,
                cpu_strategy=cfg.cpu_strategy, restrict_nodes=cfg.restrict_node_scheduling)
    for f, k in (("n_alloc", "alloc"), ("n_flags", "flags"), ("n_gpu_count", "gcount"), ("n_class", "ncls"), ("n_idle", "idle"), ("n_rel", "rel"), ("p_req", "req"),
                 ("p_class", "pcls"), ("p_nominated", "pnom"), ("p_job", "pjob"), ("class_fit", "fit"), ("perm", "perm")):
        setattr(i, f, keep[k].ctypes.data)
    q = np.ascontiguousarray(q); words = np.ascontiguousarray(words)
    out = np.zeros(len(q), A_DT)
    assert sim_lib().kai_bnsim_run(C.byref(i), q.ctypes.data, len(q), words.ctypes.data, len(words), lanes, grid, out.ctypes.data) == 0
    return out


def _cfg(strat):
    return abi.default_config(gpu_strategy=strat, cpu_strategy=strat, plugins=PLUGINS_NO_PROPORTION)


@pytest.fixture(scope="module")
def case():
    snap = the_snapshot()
    words, q = rows_and_queries(snap)
    ref = {strat: oracle_answers(snap, _cfg(strat), words, q) for strat in (abi.BINPACK, abi.SPREAD)}
    return snap, words, q, ref


@pytest.mark.parametrize("strat", [abi.BINPACK, abi.SPREAD], ids=["binpack", "spread"])
@pytest.mark.parametrize("lanes,grid", [(256, 1 << 20), (256, 7), (1, 1 << 20), (100, 3)], ids=["wg256", "grid7", "one_lane", "partial_wave"])
def test_kernel_bodies_against_the_oracle(case, strat, lanes, grid):
    snap, words, q, ref = case
    assert (np.argsort(snap.arrays["node_name_rank"]) != np.arange(snap.n_nodes)).any(), "name rank must differ from the index"
    want = ref[strat]
    assert (want["node"] >= 0).any() and (want["node"][q["nodeset"] == 0] == -1).all(), "the empty row answers -1"
    got = sim_answers(snap, _cfg(strat), words, q, lanes, grid)
    bad = np.nonzero((got["node"] != want["node"]) | (got["is_pipeline"] != want["is_pipeline"]))[0]
    assert len(bad) == 0, [(int(i), q[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


REVERSED = r'''
import json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import test_best_nodes as tb
snap = tb.the_snapshot(); words, q = tb.rows_and_queries(snap)
print(json.dumps({str(s): tb.sim_answers(snap, tb._cfg(s), words, q).tolist() for s in (tb.abi.BINPACK, tb.abi.SPREAD)}))
'''


def test_kernel_bodies_with_the_wave_order_reversed(case):
    """the emulator's waves take their turns in reverse (KW_EMU_ORDER=1, read once per process: a fresh one): a fold that leaned on the waves' order would answer differently"""
    snap, words, q, ref = case
    sim_lib()  # built before the child starts
    env = dict(os.environ, KW_EMU_ORDER="1")
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + REVERSED], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for strat in (abi.BINPACK, abi.SPREAD):
        assert [tuple(x) for x in got[str(strat)]] == [tuple(x) for x in ref[strat].tolist()], strat


def test_stand_alone_program(tmp_path):
    """the fixed case behind -DKAI_BNSIM_MAIN (the program the sanitizers are run on) builds and agrees with its serial loop"""
    exe = str(tmp_path / "best_nodes_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKAI_BNSIM_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "best_nodes_sim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
