"""kai_ordered_nodes without a GPU.

 - the export, ORDERED_MAX_K, the header text, the ABI version still 5;
 - arguments and call order under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp, as tests/test_best_nodes.py does):
   every refusal is decided before the first device call, leaves `out`, `n_out` and the session's device memory as they were and the session open; a warm handle makes
   one upload, three launches and no allocation per call, also when the calls alternate with kai_best_nodes on the scratch the two share;
 - the kernel bodies (k_bn_prep, k_bn_range, k_on_scan) run with emulated lanes by tests/host_sim/ordered_nodes_sim.cpp over arrays in name-rank order, against the
   oracle's lists.

The reference for the ORDER.  kai_oracle_best_node is the head of the list; asking it again with the winners removed from the row yields the list exactly when the
pre-order range of the bin-pack strategy (the minimum and maximum of Idle + Releasing over the node set, plugins/nodeplacement/pack.go:66-86) cannot move.  The tests make
sure of that with two ANCHOR nodes that are in every row, carry KAI_NODE_NOT_READY (they never fit, so they are never removed) and attain the minimum and the maximum:
one whose allocatable is exactly what its active pods use (Idle + Releasing = 0 with allocatable != 0), one whose allocatable is ten times the cluster's maximum.  Each
test asserts in numpy, before asking anything, that for cpu and gpu the anchors attain the row's extremes (anchors_hold).
The parity claim on the device is tests/test_gpu_ordered_nodes.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)
from test_best_nodes import A_DT, BnSimIn, Q_DT, _cfg, the_snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
RES_CPU, RES_GPU = 0, 2


def test_exports_and_header():
    assert "kai_ordered_nodes" in T.pkg.core.EXPORTS
    assert abi.ORDERED_MAX_K == 64
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    assert "int kai_ordered_nodes(" in hdr and "#define KAI_ORDERED_MAX_K 64" in hdr
    assert "with the winners removed" in hdr, "the header says why the list is not the iterated single answer"
    assert hasattr(T.pkg.load_library(), "kai_ordered_nodes")
    assert hasattr(T.pkg.core.Session, "ordered_nodes")


# ---------------------------------------------------------------------------------------------- arguments and call order
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
Q, A = abi.KaiNodeQuery, abi.KaiNodeAnswer
lib.kai_ordered_nodes.argtypes = [C.c_void_p, C.POINTER(Q), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.POINTER(A), C.POINTER(C.c_int32)]
lib.kai_best_nodes.argtypes = [C.c_void_p, C.POINTER(Q), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(A)]
snap, cfg, _ = pkg.synth.config(1, 0.3)
P, N = snap.n_pods, snap.n_nodes
W = (N + 31) // 32
SENT = 0x5a5a5a5a
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def call(h, qs, k=8, n=None, rows=2, bits=True, out=True, n_out=True):
    """qs: (pod, nodeset, flags, pad) tuples.  Returns (status, out and n_out untouched)."""
    m = max(len(qs), 1)
    arr = (Q * m)(*[Q(*q) for q in qs])
    words = (C.c_uint32 * max(rows * W, 1))(*([0xffffffff] * max(rows * W, 1)))
    kk = min(max(k, 1), 64)
    o = (A * (m * kk))(*[A(SENT, SENT) for _ in range(m * kk)])
    no = (C.c_int32 * m)(*([SENT] * m))
    rc = lib.kai_ordered_nodes(h, arr, len(qs) if n is None else n, words if bits else None, rows, k, o if out else None, no if n_out else None)
    return rc, all(x.node == SENT and x.is_pipeline == SENT for x in o) and all(x == SENT for x in no)
def best(h, qs, rows=2):
    arr = (Q * len(qs))(*[Q(*q) for q in qs])
    words = (C.c_uint32 * max(rows * W, 1))(*([0xffffffff] * max(rows * W, 1)))
    return lib.kai_best_nodes(h, arr, len(qs), words, rows, (A * len(qs))())
def cost(a, b):
    return dict(allocations=b[1] - a[1], launches=b[3] - a[3], h2d=b[4] - a[4], h2d_bytes=b[5] - a[5], d2d=b[6] - a[6], memsets=b[7] - a[7], pinned=b[8] - a[8])
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
bad["null_queries"] = (lib.kai_ordered_nodes(h, None, 2, None, 0, 8, (A * 16)(), (C.c_int32 * 2)()), True)
bad["null_out"] = call(h, good, out=False)
bad["null_n_out"] = call(h, good, n_out=False)
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
bad["k_zero"] = call(h, good, k=0)
bad["k_negative"] = call(h, good, k=-3)
bad["k_65"] = call(h, good, k=65)
bad["k_zero_without_queries"] = call(h, [], k=0)
res["bad"] = bad
# n_queries * k above 2^27: the count alone decides (the arrays are never read: four valid queries stand in front)
big = (1 << 27) // 64 + 1
qs = (Q * big)(); words = (C.c_uint32 * max(2 * W, 1))(); o1 = (A * 64)(*[A(SENT, SENT) for _ in range(64)]); n1 = (C.c_int32 * 1)(SENT)
res["capacity"] = (lib.kai_ordered_nodes(h, qs, big, words, 2, 64, o1, n1), all(x.node == SENT for x in o1) and n1[0] == SENT)
res["image_unchanged"] = image() == img0
res["empty"] = call(h, [])
res["empty_null_arrays"] = lib.kai_ordered_nodes(h, None, 0, None, 0, 1, None, None)
res["image_unchanged_by_empty"] = image() == img0
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
res["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
# good calls: what each costs on the device (the kernels of the host-only library do nothing; the counters are fake_hip's)
res["good1"] = call(h, good)[0]; i1 = image()
res["good2"] = call(h, good)[0]; i2 = image()
res["good3"] = call(h, good[:2], k=1, rows=1)[0]; i3 = image()
res["first_call"] = cost(img0, i1); res["warm_call"] = cost(i1, i2); res["smaller_call"] = cost(i2, i3)
# alternating with kai_best_nodes on the scratch the two share: a warm kai_best_nodes costs what it cost; a call that outgrows the scratch allocates and sends the
# permutation again in its one upload; the calls after it, of either kind, are warm
res["best1"] = best(h, good); i4 = image()
many = [(i % P, i % 3 - 1, i % 2, 0) for i in range(3000)]
res["grow"] = call(h, many, k=64)[0]; i5 = image()
res["best2"] = best(h, good); i6 = image()
res["again"] = call(h, many, k=64)[0]; i7 = image()
res["best3"] = best(h, good); i8 = image()
res["best_after_ordered"] = cost(i3, i4); res["grow_call"] = cost(i4, i5); res["best_after_grow"] = cost(i5, i6); res["ordered_after_best"] = cost(i6, i7); res["best_last"] = cost(i7, i8)
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
    assert out["before_open"] == [-6, True], "KAI_ERR_STATE without an open session, out and n_out untouched"
    assert out["empty_before_open"][0] == -6
    for k, (rc, untouched) in out["bad"].items():
        assert rc == -1, (k, rc)
        assert untouched, f"{k}: a refused call wrote to out or n_out"
    assert out["capacity"] == [-4, True], "KAI_ERR_CAPACITY for n_queries * k above 2^27"
    assert out["image_unchanged"], "a refused call allocated or wrote device memory"
    assert out["empty"] == [0, True] and out["empty_null_arrays"] == 0 and out["image_unchanged_by_empty"], "n_queries == 0: KAI_OK without a device call"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["sharded"] == [-5, True], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert all(out[k] == 0 for k in ("good1", "good2", "good3", "best1", "grow", "best2", "again", "best3", "still_open_after"))
    N, W = out["N"], out["W"]
    warm = dict(allocations=0, launches=3, h2d=1, d2d=0, memsets=0, pinned=0)
    def is_warm(c, queries, rows):
        return {k: v for k, v in c.items() if k != "h2d_bytes"} == warm and c["h2d_bytes"] < queries * 16 + rows * 4 * W + (rows + 1) * 8 + 64
    # one upload, three launches (the default configuration bin-packs: the range kernel runs); the first call of a session allocates the scratch and sends the permutation
    f = out["first_call"]
    assert f["launches"] == 3 and f["h2d"] == 1 and f["allocations"] == 1 and f["h2d_bytes"] >= 4 * N + 4 * 16 + 2 * 4 * W
    assert is_warm(out["warm_call"], 4, 2), out["warm_call"]
    assert is_warm(out["smaller_call"], 2, 1), out["smaller_call"]
    # kai_best_nodes' own cost on the shared scratch: what tests/test_best_nodes.py pins
    assert is_warm(out["best_after_ordered"], 4, 2), out["best_after_ordered"]
    g = out["grow_call"]
    # (the counters are of live allocations: a buffer that grows is released and allocated, net 0)
    assert g["launches"] == 3 and g["h2d"] == 1 and g["h2d_bytes"] >= 4 * N + 3000 * 16, "a grown scratch gets the permutation again, in the one upload"
    assert is_warm(out["best_after_grow"], 4, 2), out["best_after_grow"]
    assert is_warm(out["ordered_after_best"], 3000, 2), out["ordered_after_best"]
    assert is_warm(out["best_last"], 4, 2), out["best_last"]


# ---------------------------------------------------------------------------------------------- the anchored reference lists
def idle_plus_releasing(snap):
    """[R][N] Idle + Releasing a fresh open would hold, caller's node indices (node_info.go:457-493)"""
    a = snap.arrays
    st, nd = a["pod_status"], a["pod_node"]
    idle, rel = a["node_allocatable"].astype(np.float64).copy(), np.zeros_like(a["node_allocatable"], dtype=np.float64)
    releasing, pipelined = st == abi.POD_STATUS["Releasing"], st == abi.POD_STATUS["Pipelined"]
    taking = ((st & abi.ACTIVE_USED) != 0) & ~pipelined & (nd >= 0)
    for r in range(snap.n_res):
        np.subtract.at(idle[r], nd[taking], a["pod_req"][r, taking])
        np.add.at(rel[r], nd[releasing & (nd >= 0)], a["pod_req"][r, releasing & (nd >= 0)])
        np.subtract.at(rel[r], nd[pipelined & (nd >= 0)], a["pod_req"][r, pipelined & (nd >= 0)])
    return idle + rel


def add_anchors(snap):
    """Turns the first and the last node that have cpu and gpu in use (and no Releasing or Pipelined pod) into the anchors, in place.  Returns (low, high), caller's indices."""
    a = snap.arrays
    st, nd = a["pod_status"], a["pod_node"]
    soft = (st == abi.POD_STATUS["Releasing"]) | (st == abi.POD_STATUS["Pipelined"])
    taking = ((st & abi.ACTIVE_USED) != 0) & (nd >= 0)
    used = np.zeros_like(a["node_allocatable"], dtype=np.float64)
    for r in range(snap.n_res):
        np.add.at(used[r], nd[taking], a["pod_req"][r, taking])
    quiet = np.ones(snap.n_nodes, bool); quiet[nd[soft & (nd >= 0)]] = False
    both = np.nonzero((used[RES_CPU] > 0) & (used[RES_GPU] > 0) & quiet)[0]
    assert len(both) >= 2, "the snapshot has no two nodes to anchor"
    lo, hi = int(both[0]), int(both[-1])
    top = a["node_allocatable"].max(axis=1)
    a["node_allocatable"][:, lo] = used[:, lo]
    a["node_allocatable"][:, hi] = 10 * top
    a["node_flags"][[lo, hi]] |= abi.NODE_NOT_READY
    return lo, hi


def anchors_hold(alloc, ipr, masks, lo, hi):
    """for cpu and gpu the anchors attain every row's minimum and maximum of Idle + Releasing over the nodes with allocatable != 0 (alloc, ipr: [R][N], caller's indices)"""
    for m in list(masks) + [np.ones(alloc.shape[1], bool)]:
        if not (m[lo] and m[hi]): return False
        for r in (RES_CPU, RES_GPU):
            sel = m & (alloc[r] != 0)
            if not (sel[lo] and sel[hi] and ipr[r][lo] == 0 and ipr[r][lo] == ipr[r][sel].min() and ipr[r][hi] == ipr[r][sel].max()): return False
    return True


def words_of(masks, N):
    w = np.zeros((max(len(masks), 1), max((N + 31) // 32, 1)), np.uint32)
    for s, m in enumerate(masks):
        idx = np.nonzero(m)[0]
        np.bitwise_or.at(w[s], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return w


def oracle_lists(snap, cfg, masks, q, k):
    """per query the list of up to k (node, is_pipeline): kai_oracle_best_node asked again and again with the winners removed from the row"""
    lib = T.Oracle.lib(); lib.kai_oracle_best_node.restype = C.c_int
    s = snap.as_struct()
    N = snap.n_nodes
    words, full = words_of(masks, N), words_of([np.ones(N, bool)], N)[0]
    memo = {}
    for x in q:
        key = (int(x["pod"]), int(x["nodeset"]), int(x["flags"]))
        if key in memo: continue
        row = np.ascontiguousarray(full if key[1] < 0 else words[key[1]]).copy()
        lst = []
        while len(lst) < k:
            node, pipe = C.c_int(-1), C.c_int(0)
            assert lib.kai_oracle_best_node(C.byref(cfg), C.byref(s), key[0], row.ctypes.data_as(C.POINTER(C.c_uint32)), key[2] & 1, C.byref(node), C.byref(pipe)) == 0
            if node.value < 0: break
            lst.append((node.value, pipe.value))
            row[node.value >> 5] &= ~(np.uint32(1) << np.uint32(node.value & 31))
        memo[key] = lst
    return [memo[(int(x["pod"]), int(x["nodeset"]), int(x["flags"]))] for x in q]


def as_lists(node, pipe, count):
    """what the call returned as lists of (node, is_pipeline); asserts that the entries behind a list's end are {-1, 0}"""
    node, pipe, count = np.asarray(node), np.asarray(pipe).astype(int), np.asarray(count)
    k = node.shape[1]
    tail = np.arange(k)[None, :] >= count[:, None]
    assert (count >= 0).all() and (count <= k).all() and (node[tail] == -1).all() and (pipe[tail] == 0).all() and (node[~tail] >= 0).all(), "entries j >= n_out[i] are {-1, 0}"
    return [list(zip(node[i, :c].tolist(), pipe[i, :c].tolist())) for i, c in enumerate(count.tolist())]


def anchored_case(n_pods=16, seed=5):
    """the_snapshot() with anchors; rows of density 0, 0.02, 0.2, 0.7 and 1, each with the anchors; a query per row and one over all nodes for n_pods pending pods,
    every third PIPELINE_ONLY"""
    snap = the_snapshot()
    lo, hi = add_anchors(snap)
    rng = np.random.default_rng(seed)
    N = snap.n_nodes
    masks = [rng.random(N) < d for d in (0.0, 0.02, 0.2, 0.7)] + [np.ones(N, bool)]
    for m in masks: m[[lo, hi]] = True
    assert anchors_hold(snap.arrays["node_allocatable"], idle_plus_releasing(snap), masks, lo, hi)
    pending = np.nonzero(snap.arrays["pod_status"] == abi.POD_STATUS["Pending"])[0]
    pods = rng.choice(pending, size=n_pods, replace=False)
    q = np.zeros(n_pods * (len(masks) + 1), Q_DT)
    q["pod"] = np.repeat(pods, len(masks) + 1)
    q["nodeset"] = np.tile(np.arange(-1, len(masks)), n_pods)
    q["flags"] = (np.arange(len(q)) % 3 == 0).astype(np.uint32)
    return snap, masks, q


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "ordered_nodes_sim.cpp")


def sim_lib():
    import glob
    so = os.path.join(ROOT, "tests", "host_sim", "liborderednodessim.so")
    deps = [SIM_SRC, os.path.join(ROOT, "tests", "host_sim", "best_nodes_sim.cpp")] + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_onsim_run.restype = C.c_int
    lib.kai_onsim_run.argtypes = [C.POINTER(BnSimIn), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.kai_bnsim_run.restype = C.c_int
    lib.kai_bnsim_run.argtypes = [C.POINTER(BnSimIn), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return lib


def sim_input(snap, cfg):
    """The session state a fresh open would hold, in numpy: nodes in name-rank order (as tests/test_best_nodes.py sim_answers builds it).  Returns (BnSimIn, what it points into)."""
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
    return i, keep


def sim_lists(snap, cfg, masks, q, k, lanes=256, grid=1 << 20):
    i, _keep = sim_input(snap, cfg)
    q = np.ascontiguousarray(q); words = np.ascontiguousarray(words_of(masks, snap.n_nodes))
    out = np.zeros((len(q), k), A_DT); n_out = np.zeros(len(q), np.int32)
    assert sim_lib().kai_onsim_run(C.byref(i), q.ctypes.data, len(q), words.ctypes.data, len(masks), k, lanes, grid, out.ctypes.data, n_out.ctypes.data) == 0
    return as_lists(out["node"], out["is_pipeline"], n_out)


def sim_best(snap, cfg, masks, q):
    i, _keep = sim_input(snap, cfg)
    q = np.ascontiguousarray(q); words = np.ascontiguousarray(words_of(masks, snap.n_nodes))
    out = np.zeros(len(q), A_DT)
    assert sim_lib().kai_bnsim_run(C.byref(i), q.ctypes.data, len(q), words.ctypes.data, len(masks), 256, 1 << 20, out.ctypes.data) == 0
    return out


@pytest.fixture(scope="module")
def case():
    snap, masks, q = anchored_case()
    ref = {strat: oracle_lists(snap, _cfg(strat), masks, q, abi.ORDERED_MAX_K) for strat in (abi.BINPACK, abi.SPREAD)}  # (a list of k is the head of the list of 64)
    return snap, masks, q, ref


def test_the_reference_lists_are_worth_comparing(case):
    snap, masks, q, ref = case
    assert (np.argsort(snap.arrays["node_name_rank"]) != np.arange(snap.n_nodes)).any(), "name rank must differ from the index"
    for strat, lists in ref.items():
        lens = {min(len(l), 8) for l in lists}
        assert 0 in lens and 8 in lens and len(lens) >= 4, "exhausted and full lists both occur at k = 8"
        assert all(len(l) == 0 for l, x in zip(lists, q) if x["nodeset"] == 0), "a row of the anchors alone answers nothing"
        assert any(len(l) > 8 for l in lists)


@pytest.mark.parametrize("strat", [abi.BINPACK, abi.SPREAD], ids=["binpack", "spread"])
@pytest.mark.parametrize("k", [1, 2, 8, 64])
@pytest.mark.parametrize("lanes,grid", [(256, 1 << 20), (256, 3), (64, 1 << 20), (128, 2)], ids=["wg256", "grid3", "one_wave", "two_waves"])
def test_kernel_bodies_against_the_oracle_lists(case, strat, k, lanes, grid):
    snap, masks, q, ref = case
    want = [l[:k] for l in ref[strat]]
    got = sim_lists(snap, _cfg(strat), masks, q, k, lanes, grid)
    bad = [i for i in range(len(q)) if got[i] != want[i]]
    assert not bad, [(i, q[i].tolist(), got[i], want[i]) for i in bad[:4]]
    if k == 1 and lanes == 256:  # answer for answer kai_best_nodes' kernels
        b = sim_best(snap, _cfg(strat), masks, q)
        assert [([(int(x["node"]), int(x["is_pipeline"]))] if x["node"] >= 0 else []) for x in b] == got
        assert all(x["is_pipeline"] == 0 for x in b if x["node"] < 0)


REVERSED = r'''
import json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import test_ordered_nodes as to
snap, masks, q = to.anchored_case()
print(json.dumps({f"{s}/{k}": to.sim_lists(snap, to._cfg(s), masks, q, k) for s in (to.abi.BINPACK, to.abi.SPREAD) for k in (2, 64)}))
'''


def test_kernel_bodies_with_the_wave_order_reversed(case):
    """the emulator's waves take their turns in reverse (KW_EMU_ORDER=1, read once per process: a fresh one): a merge that leaned on the waves' order would answer differently"""
    snap, masks, q, ref = case
    sim_lib()  # built before the child starts
    env = dict(os.environ, KW_EMU_ORDER="1")
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + REVERSED], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for strat in (abi.BINPACK, abi.SPREAD):
        for k in (2, 64):
            assert [[tuple(e) for e in l] for l in got[f"{strat}/{k}"]] == [l[:k] for l in ref[strat]], (strat, k)


def test_stand_alone_program(tmp_path):
    """the fixed case behind -DKAI_ONSIM_MAIN (the program the sanitizers are run on) builds and agrees with its serial sort"""
    exe = str(tmp_path / "ordered_nodes_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKAI_ONSIM_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ordered_nodes_sim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
