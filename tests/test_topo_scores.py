"""kai_subset_nodes_scored and kai_ordered_nodes_scored without a GPU.

 - the exports, the ABI structs and constants, the header text, the ABI version still 5;
 - arguments under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp): every refusal of both calls is made before the first
   device call and leaves the device memory image, the session and the caller's arrays as they were; n_queries == 0 is KAI_OK without a device call; a warm call costs what
   the unscored call costs (launches, uploads, allocations);
 - the kernel bodies (kai_subset_nodes.hpp with want_scores, both paths; k_on_scan_scored) run with emulated lanes by tests/host_sim/topo_scores_sim.cpp on a session of the
   host simulation that lives across the calls.

The reference for the SCORES is the oracle's calculateNodeScores (kai_oracle_topology_scores: per node, the job's root sub-group over all nodes; pinned on the reference's
TestCalculateNodeScores by tests/test_oracle_topology_kat.py).  A call's row is expanded through node_domain[level_row] to per-node scores and must equal it, -1 = no score
included.  Where the reference's function returns an error (KAI_SUBSET_BAD_LEVEL) the oracle's export has nothing to read: there the two paths are held against each other.
The reference for the ORDER a gang is placed in is the oracle's allocate action (kai_oracle_run).  The parity claim on the device is tests/test_gpu_topo_scores.py."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
import test_oracle_topology_kat as KAT
from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)
from test_ordered_nodes import as_lists, words_of
from test_subset_nodes import (A_DT, BAD_LEVEL, ENGINE, NO_FIT, OK, Q_DT, S_DT, SHAPES, WIDE, check_consistent, inner_walk, kat_scenes, oracle_answer, replica_scene,
                               same_answers, synthetic, topology_jobs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
NONE_ROW, EMPTY_ROW, NO_SCORE = abi.TOPO_SCORES_NONE, abi.TOPO_SCORES_EMPTY, abi.TOPO_NO_SCORE
R_DT = np.dtype([("level_row", "<i4"), ("n_scored", "<i4")])
SQ_DT = np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("scores", "<i4")])
NA_DT = np.dtype([("node", "<i4"), ("is_pipeline", "<i4")])


def test_exports_and_struct_sizes():
    assert "kai_subset_nodes_scored" in T.pkg.core.EXPORTS and "kai_ordered_nodes_scored" in T.pkg.core.EXPORTS
    assert C.sizeof(abi.KaiTopoScoreRow) == 8 and C.sizeof(abi.KaiScoredQuery) == 16 and abi.KaiScoredQuery.scores.offset == 12
    assert [f[0] for f in abi.KaiTopoScoreRow._fields_] == list(R_DT.names) and [f[0] for f in abi.KaiScoredQuery._fields_] == list(SQ_DT.names)
    assert [f[0] for f in abi.KaiScoredQuery._fields_][:3] == [f[0] for f in abi.KaiNodeQuery._fields_][:3], "kai_node_query's layout with scores in place of pad"
    assert (abi.TOPO_SCORE_UNIT, NO_SCORE, NONE_ROW, EMPTY_ROW) == (10000.0, 255, -1, -2)
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    for text in ("#define KAI_TOPO_SCORE_UNIT   10000.0", "#define KAI_TOPO_NO_SCORE     255", "#define KAI_TOPO_SCORES_NONE  (-1)", "#define KAI_TOPO_SCORES_EMPTY (-2)",
                 "typedef struct kai_topo_score_row { int32_t level_row; int32_t n_scored; } kai_topo_score_row;",
                 "typedef struct kai_scored_query { int32_t pod; int32_t nodeset; uint32_t flags; int32_t scores; } kai_scored_query;",
                 "int kai_subset_nodes_scored(kai_core* core, const kai_subset_params* params,", "int kai_ordered_nodes_scored(kai_core* core, const kai_scored_query* queries, int32_t n_queries,",
                 "nearest ancestor", "node_scoring.go:37-53"):
        assert text in hdr, text
    assert "a query there is scored without a topology term.  Out of scope of this call." not in hdr, "the sentence about the missing scores is replaced by a pointer to the new call"
    lib = T.pkg.load_library()
    assert hasattr(lib, "kai_subset_nodes_scored") and hasattr(lib, "kai_ordered_nodes_scored")
    assert hasattr(T.pkg.core.Session, "subset_nodes_scored") and hasattr(T.pkg.core.Session, "ordered_nodes_scored")
    for doc, word in (("INTEGRATION.md", "kai_subset_nodes_scored"), ("DESIGN.md", "k_on_scan_scored"), ("README.md", "kai_ordered_nodes_scored")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
    assert "func SubsetNodesScored(" in open(os.path.join(ROOT, "shim", "kai_cgo.go")).read() and "func OrderedNodesScored(" in open(os.path.join(ROOT, "shim", "kai_cgo.go")).read()


# ---------------------------------------------------------------------------------------------- arguments and refusals under the host-only library
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
import test_subset_nodes as ts
import test_topo_scores as tt
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
I64 = C.POINTER(C.c_int64)
lib.kai_subset_nodes_scored.argtypes = [C.c_void_p, C.POINTER(abi.KaiSubsetParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, I64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.KaiSubsetResult)]
lib.kai_subset_nodes.argtypes = [C.c_void_p, C.POINTER(abi.KaiSubsetParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, I64, C.c_void_p, C.POINTER(abi.KaiSubsetResult)]
lib.kai_ordered_nodes_scored.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
lib.kai_ordered_nodes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
snap, cfg = ts.replica_scene()
a = snap.arrays
N, W, P, D, TL = snap.n_nodes, (snap.n_nodes + 31) // 32, snap.n_pods, len(a["domain_parent"]), int(a["node_domain"].shape[0])
child = int(np.nonzero(a["group_parent"] >= 0)[0][0]); cj = int(a["group_job"][child]); other = int(np.nonzero(a["group_job"] != cj)[0][0])
cps = int(np.nonzero(a["podset_group"] == child)[0][0]); ops = int(np.nonzero(a["podset_job"] != cj)[0][0])
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def subset(h, version=1, flags=0, q=((0, -1, -1, -1),), n_rows=0, cap=64, null=(), m=None, scored=True):
    """-> [status, every output untouched, n_sets_out]"""
    qa = np.array(list(q), ts.Q_DT); M = len(qa) if m is None else m
    ans = np.full(max(len(qa), 1) * 6, -7, np.int32); sets = np.full(64 * 4, -8, np.int32); maps = np.full(64 * max(W, 1), 0x99, np.uint32); rows = np.zeros(max(n_rows, 1) * max(W, 1), np.uint32)
    sr = np.full(max(len(qa), 1) * 2, -9, np.int32); dec = np.full(max(len(qa), 1) * max(D, 1), 0x66, np.uint8)
    n = C.c_int64(-3); r = abi.KaiSubsetResult(11, 12, 13); pm = abi.KaiSubsetParams(version, flags)
    head = [h, None if "params" in null else C.byref(pm), None if "queries" in null else qa.ctypes.data, M, None if "rows" in null else rows.ctypes.data, n_rows,
            None if "answers" in null else ans.ctypes.data, None if "sets" in null else sets.ctypes.data, cap, None if "n" in null else C.byref(n), None if "maps" in null else maps.ctypes.data]
    tail = [None if "result" in null else C.byref(r)]
    rc = lib.kai_subset_nodes_scored(*head, None if "score_rows" in null else sr.ctypes.data, None if "deciles" in null else dec.ctypes.data, *tail) if scored else lib.kai_subset_nodes(*head, *tail)
    untouched = bool((ans == -7).all() and (sets == -8).all() and (maps == 0x99).all() and (sr == -9).all() and (dec == 0x66).all() and n.value == -3 and (r.n_sets, r.path, r.pad) == (11, 12, 13))
    return [rc, untouched, n.value]
SENT = 0x5a5a5a5a
def ordered(h, qs, k=8, n=None, rows=2, bits=True, out=True, n_out=True, srows=((0, 1), (-1, 0), (-2, 0)), n_srows=None, dec=None, null=(), scored=True):
    """qs: (pod, nodeset, flags, scores) tuples.  Returns [status, out and n_out untouched]."""
    m = max(len(qs), 1)
    arr = np.array(list(qs) if len(qs) else [(0, -1, 0, -1)], tt.SQ_DT)
    words = np.full(max(rows * W, 1), 0xffffffff, np.uint32)
    kk = min(max(k, 1), 64)
    o = np.full(m * kk * 2, SENT, np.int32); no = np.full(m, SENT, np.int32)
    sr = np.array(list(srows) if len(srows) else [(0, 0)], tt.R_DT)
    dd = np.full((len(sr), max(D, 1)), 255, np.uint8) if dec is None else dec
    ns = len(srows) if n_srows is None else n_srows
    if scored:
        rc = lib.kai_ordered_nodes_scored(h, None if "queries" in null else arr.ctypes.data, len(qs) if n is None else n, words.ctypes.data if bits else None, rows,
                                          None if "score_rows" in null else sr.ctypes.data, None if "deciles" in null else dd.ctypes.data, ns, k, o.ctypes.data if out else None, no.ctypes.data if n_out else None)
    else:
        arr["scores"] = 0
        rc = lib.kai_ordered_nodes(h, arr.ctypes.data, len(qs), words.ctypes.data, rows, k, o.ctypes.data, no.ctypes.data)
    return [rc, bool((o == SENT).all() and (no == SENT).all())]
def cost(x, y):
    return dict(allocations=y[1] - x[1], launches=y[3] - x[3], h2d=y[4] - x[4], memsets=y[7] - x[7], pinned=y[8] - x[8])
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
good = [(0, -1, 0, -1), (1, 0, 1, 0), (P - 1, 1, 0, 1), (1, 0, 1, 2)]
res["subset_before_open"] = subset(h); res["ordered_before_open"] = ordered(h, good)
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = image()
bad = {}
bad["version"] = subset(h, version=2)
bad["unknown_flags"] = subset(h, flags=2)
bad["unknown_flags_high"] = subset(h, flags=0x80000001)
bad["null_params"] = subset(h, null=("params",))
bad["null_n_sets_out"] = subset(h, null=("n",))
bad["null_queries"] = subset(h, null=("queries",))
bad["null_answers"] = subset(h, null=("answers",))
bad["null_rows_with_count"] = subset(h, n_rows=1, null=("rows",))
bad["null_sets_with_capacity"] = subset(h, null=("sets",))
bad["null_score_rows"] = subset(h, null=("score_rows",))
bad["null_deciles"] = subset(h, null=("deciles",))
bad["negative_queries"] = subset(h, m=-1)
bad["negative_rows"] = subset(h, n_rows=-1)
bad["negative_capacity"] = subset(h, cap=-1)
bad["job_high"] = subset(h, q=((snap.n_jobs, -1, -1, -1),))
bad["job_negative"] = subset(h, q=((-1, -1, -1, -1),))
bad["group_high"] = subset(h, q=((cj, len(a["group_job"]), -1, -1),))
bad["group_below"] = subset(h, q=((cj, -2, -1, -1),))
bad["podset_high"] = subset(h, q=((cj, -1, snap.n_podsets, -1),))
bad["group_of_another_job"] = subset(h, q=((other, child, -1, -1),))
bad["podset_of_another_job"] = subset(h, q=((cj, -1, ops, -1),))
bad["group_and_podset"] = subset(h, q=((cj, child, cps, -1),))
bad["nodeset_high"] = subset(h, q=((0, -1, -1, 1),), n_rows=1)
bad["nodeset_below"] = subset(h, q=((0, -1, -1, -2),))
bad["second_query_bad"] = subset(h, q=((0, -1, -1, -1), (snap.n_jobs, -1, -1, -1)))
res["bad_subset"] = bad
bad = {}
bad["null_queries"] = ordered(h, good, null=("queries",))
bad["null_out"] = ordered(h, good, out=False)
bad["null_n_out"] = ordered(h, good, n_out=False)
bad["null_bitmaps"] = ordered(h, good, bits=False)
bad["negative_queries"] = ordered(h, good, n=-1)
bad["negative_nodesets"] = ordered(h, [(0, -1, 0, -1)], rows=-1)
bad["pod_negative"] = ordered(h, good + [(-1, -1, 0, -1)])
bad["pod_too_large"] = ordered(h, good + [(P, -1, 0, -1)])
bad["nodeset_too_large"] = ordered(h, good + [(0, 2, 0, -1)])
bad["nodeset_below_minus_one"] = ordered(h, good + [(0, -2, 0, -1)])
bad["unknown_flags"] = ordered(h, good + [(0, -1, 2, -1)])
bad["unknown_flags_high"] = ordered(h, [(0, -1, 0x80000001, -1)] + good)
bad["k_zero"] = ordered(h, good, k=0)
bad["k_65"] = ordered(h, good, k=65)
bad["k_zero_without_queries"] = ordered(h, [], k=0)
bad["scores_high"] = ordered(h, good + [(0, -1, 0, 3)])
bad["scores_below_minus_one"] = ordered(h, good + [(0, -1, 0, -2)])
bad["scores_without_rows"] = ordered(h, [(0, -1, 0, 0)], srows=(), n_srows=0)
bad["negative_score_rows"] = ordered(h, [(0, -1, 0, -1)], n_srows=-1)
bad["null_score_rows"] = ordered(h, good, null=("score_rows",))
bad["null_deciles"] = ordered(h, good, null=("deciles",))
bad["level_row_high"] = ordered(h, good, srows=((0, 1), (TL, 0), (-2, 0)))
bad["level_row_below_minus_two"] = ordered(h, good, srows=((0, 1), (-3, 0), (-2, 0)))
d11 = np.full((3, max(D, 1)), 255, np.uint8); d11[2, D - 1] = 11
d254 = np.full((3, max(D, 1)), 255, np.uint8); d254[0, 0] = 254
bad["decile_11"] = ordered(h, good, dec=d11)
bad["decile_254"] = ordered(h, good, dec=d254)
bad["bad_rows_without_queries"] = ordered(h, [], dec=d11)
res["bad_ordered"] = bad
big = (1 << 27) // 64 + 1
qs = np.zeros(big, tt.SQ_DT); qs["nodeset"] = -1; qs["scores"] = -1
o1 = np.full(128, SENT, np.int32); n1 = np.full(1, SENT, np.int32); words = np.zeros(max(2 * W, 1), np.uint32)
res["capacity"] = [lib.kai_ordered_nodes_scored(h, qs.ctypes.data, big, words.ctypes.data, 2, None, None, 0, 64, o1.ctypes.data, n1.ctypes.data), bool((o1 == SENT).all() and n1[0] == SENT)]
res["image_unchanged"] = image() == img0
res["subset_empty"] = subset(h, q=(), m=0, null=("queries", "answers", "sets", "maps", "rows", "score_rows", "deciles"), cap=0)
res["ordered_empty"] = ordered(h, [])
res["ordered_empty_null_arrays"] = lib.kai_ordered_nodes_scored(h, None, 0, None, 0, None, None, 0, 1, None, None)
res["image_unchanged_by_empty"] = image() == img0
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
res["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
# calls that go through (the kernels of the host-only library do nothing); what each costs on the device, beside the unscored calls
q3 = ((cj, child, -1, -1), (cj, -1, cps, 0), (0, -1, -1, -1))
res["s1"] = subset(h, q=q3, n_rows=1); i1 = image()
res["s2"] = subset(h, q=q3, n_rows=1); i2 = image()
res["u1"] = subset(h, q=q3, n_rows=1, scored=False); i3 = image()
res["u2"] = subset(h, q=q3, n_rows=1, scored=False); i4 = image()
res["s3"] = subset(h, q=q3, n_rows=1, flags=1); i5 = image()
res["subset_first"] = cost(img0, i1); res["subset_warm"] = cost(i1, i2); res["subset_unscored_warm"] = cost(i3, i4); res["subset_engine"] = cost(i4, i5)
res["o1"] = ordered(h, good); j1 = image()
res["o2"] = ordered(h, good); j2 = image()
res["p1"] = ordered(h, good, scored=False); j3 = image()
res["p2"] = ordered(h, good, scored=False); j4 = image()
res["o3"] = ordered(h, [(0, -1, 0, -1)], srows=(), n_srows=0, null=("score_rows", "deciles")); j5 = image()
res["ordered_first"] = cost(i5, j1); res["ordered_warm"] = cost(j1, j2); res["ordered_unscored_warm"] = cost(j3, j4); res["ordered_without_rows"] = cost(j4, j5)
lib.kai_core_destroy(h)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["subset_sharded"] = subset(h2); res["ordered_sharded"] = ordered(h2, good)
lib.kai_core_destroy(h2)
print(json.dumps(res))
'''


def test_arguments_and_refusals(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["subset_before_open"][:2] == [-6, True] and out["ordered_before_open"] == [-6, True], "KAI_ERR_STATE without an open session"
    for which in ("bad_subset", "bad_ordered"):
        for k, v in out[which].items():
            assert v[:2] == [-1, True], (which, k, v)
    assert out["capacity"] == [-4, True], "KAI_ERR_CAPACITY for n_queries * k above 2^27"
    assert out["image_unchanged"], "a refused call allocated or wrote device memory"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["subset_sharded"][:2] == [-5, True] and out["ordered_sharded"] == [-5, True], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["subset_empty"][0] == 0 and out["subset_empty"][2] == 0 and out["ordered_empty"] == [0, True] and out["ordered_empty_null_arrays"] == 0 and out["image_unchanged_by_empty"], \
        "n_queries == 0: KAI_OK without a device call"
    for k in ("s1", "s2", "u1", "u2", "s3", "o1", "o2", "p1", "p2", "o3"):
        assert out[k][0] == 0, (k, out[k])
    # the figures of the unscored calls (tests/test_subset_nodes.py, tests/test_ordered_nodes.py): a call whose total is 0 makes one upload and the chunk, prep, walk and offsets
    # launches; a list call one upload and three launches; no allocation on a warm handle
    assert out["subset_first"]["launches"] == 4 and out["subset_first"]["h2d"] == 1
    warm4 = dict(allocations=0, launches=4, h2d=1, memsets=0, pinned=0)
    assert out["subset_warm"] == warm4 and out["subset_unscored_warm"] == warm4, (out["subset_warm"], out["subset_unscored_warm"])
    assert out["subset_engine"]["launches"] == 4 and out["subset_engine"]["h2d"] == 1 and out["subset_engine"]["allocations"] == 0, out["subset_engine"]
    assert out["ordered_first"]["launches"] == 3 and out["ordered_first"]["h2d"] == 1
    warm3 = dict(allocations=0, launches=3, h2d=1, memsets=0, pinned=0)
    assert out["ordered_warm"] == warm3 and out["ordered_unscored_warm"] == warm3 and out["ordered_without_rows"] == warm3, (out["ordered_warm"], out["ordered_unscored_warm"], out["ordered_without_rows"])


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes, on a session that lives across the calls
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "topo_scores_sim.cpp")
ACTIONS = {"allocate": 0}


def sim_lib():
    so = os.path.join(ROOT, "tests", "host_sim", "libtoposcoressim.so")
    deps = glob.glob(os.path.join(ROOT, "tests", "host_sim", "*.?pp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_tssim_open.restype = C.c_void_p
    lib.kai_tssim_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.kai_tssim_close.restype = None
    lib.kai_tssim_close.argtypes = [C.c_void_p]
    lib.kai_tssim_action.argtypes = [C.c_void_p, C.c_int]
    lib.kai_tssim_subset.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(abi.KaiSubsetResult), C.POINTER(C.c_int)]
    lib.kai_tssim_ordered.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.kai_tssim_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.kai_tssim_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    return lib


class Sim:
    """a session of the host simulation: the two calls, actions, kai_ops_apply and the read-back on it"""

    def __init__(self, snap, cfg, n_actions=1):
        self.lib, self.snap, self.cfg, self.struct = sim_lib(), snap, cfg, snap.as_struct()
        rc = C.c_int(0)
        self.h = self.lib.kai_tssim_open(C.addressof(cfg), C.addressof(self.struct), n_actions, C.byref(rc))
        assert self.h and rc.value == 0, rc.value
        self.D = len(snap.arrays["domain_parent"]) if "domain_parent" in snap.arrays else 0

    def __enter__(self): return self

    def __exit__(self, *exc): self.lib.kai_tssim_close(self.h); self.h = None

    def action(self, name): assert self.lib.kai_tssim_action(self.h, ACTIONS[name]) == 0

    def subset(self, jobs, groups=None, podsets=None, rows=None, nodeset_of=None, engine=False, scored=True, lanes=256, wgs=1 << 20):
        snap = self.snap
        N, W, M, D = snap.n_nodes, max((snap.n_nodes + 31) // 32, 1), len(jobs), self.D
        per = lambda v: np.full(M, -1, np.int32) if v is None else np.asarray(v, np.int32)
        q = np.zeros(M, Q_DT); q["job"], q["group"], q["podset"], q["nodeset"] = np.asarray(jobs, np.int32), per(groups), per(podsets), per(nodeset_of)
        rows = [] if rows is None else list(rows)
        words = np.ascontiguousarray(words_of(rows, N))
        cap = M * (D + 2)
        ans = np.zeros(max(M, 1), A_DT); sets = np.zeros(max(cap, 1), S_DT); maps = np.zeros((max(cap, 1), W), np.uint32)
        sr = np.full(max(M, 1), -77, R_DT); dec = np.full((max(M, 1), max(D, 1)), 0x77, np.uint8)
        n, res, same = C.c_int64(0), abi.KaiSubsetResult(), C.c_int(0)
        status = self.lib.kai_tssim_subset(self.h, 1 if scored else 0, abi.SUBSET_ENGINE_PATH if engine else 0, lanes, wgs, q.ctypes.data, M, words.ctypes.data, len(rows), ans.ctypes.data,
                                           sets.ctypes.data, cap, C.byref(n), maps.ctypes.data, sr.ctypes.data, dec.ctypes.data, C.byref(res), C.byref(same))
        total = int(n.value)
        bits = (maps[:total, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
        return T.Result(q=q, rows=rows, call_status=status, ans=ans[:M], sets=sets[:total].copy(), masks=bits.reshape(total, W * 32)[:, :N].astype(bool), res=res, unchanged=same.value,
                        score_rows=sr[:M], deciles=np.ascontiguousarray(dec[:M, :D]))

    def ordered(self, pods, k, rows=None, nodeset_of=None, score_rows=None, deciles=None, scores_of=None, flags=None, scored=True, lanes=256, grid=1 << 20):
        """-> lists of (node, is_pipeline) per pod"""
        M, N = len(pods), self.snap.n_nodes
        q = np.zeros(M, SQ_DT); q["pod"] = np.asarray(pods, np.int32); q["nodeset"] = -1 if nodeset_of is None else np.asarray(nodeset_of, np.int32)
        q["flags"] = 0 if flags is None else np.asarray(flags, np.uint32)
        q["scores"] = (-1 if scores_of is None else np.asarray(scores_of, np.int32)) if scored else 0
        rows = [] if rows is None else list(rows)
        words = np.ascontiguousarray(words_of(rows, N))
        sr = np.zeros(1, R_DT) if score_rows is None else np.ascontiguousarray(score_rows, dtype=R_DT)
        n_sr = 0 if score_rows is None else len(sr)
        dec = np.zeros((1, max(self.D, 1)), np.uint8) if deciles is None else np.ascontiguousarray(deciles, dtype=np.uint8)
        out = np.zeros((M, k), NA_DT); n_out = np.zeros(max(M, 1), np.int32)
        assert self.lib.kai_tssim_ordered(self.h, 1 if scored else 0, q.ctypes.data, M, words.ctypes.data, len(rows), sr.ctypes.data, dec.ctypes.data, n_sr, k, lanes, grid, out.ctypes.data, n_out.ctypes.data) == 0
        return as_lists(out["node"], out["is_pipeline"], n_out[:M])

    def apply(self, ops):
        arr = np.ascontiguousarray(ops, dtype=T.pkg.core._OP_DTYPE)
        assert self.lib.kai_tssim_apply(self.h, arr.ctypes.data, len(arr)) == 0

    def state(self):
        P = self.snap.n_pods
        st, nd, ops, n = np.zeros(max(P, 1), np.int32), np.zeros(max(P, 1), np.int32), np.zeros(8 * P + 64, T.pkg.core._OP_DTYPE), C.c_int64(0)
        assert self.lib.kai_tssim_state(self.h, st.ctypes.data, nd.ctypes.data, ops.ctypes.data, len(ops), C.byref(n)) == 0
        return st[:P], nd[:P], ops[:n.value].copy()


def node_scores(snap, row, dec):
    """a call's score row expanded through node_domain[level_row]: the score per node, -1 = none"""
    out = np.full(snap.n_nodes, -1.0)
    if row["level_row"] >= 0:
        dd = snap.arrays["node_domain"][int(row["level_row"])]
        d = dec[np.maximum(dd, 0)]
        has = (dd >= 0) & (d != NO_SCORE)
        out[has] = d[has] * abi.TOPO_SCORE_UNIT
    return out


def oracle_scores(snap, cfg, job):
    """what t.subGroupNodeScores[root sub-group] gives every node after subSetNodesFn over all nodes, -1 = no score; None where the function returns an error"""
    lib = T.Oracle.lib(); lib.kai_oracle_topology_scores.restype = C.c_int
    out = np.zeros(max(snap.n_nodes, 1)); s = snap.as_struct()
    rc = lib.kai_oracle_topology_scores(C.byref(cfg), C.byref(s), int(job), out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc in (0, -1), rc
    return out[:snap.n_nodes] if rc == 0 else None


def check_rows(snap, r, what=""):
    """what holds of every score row: a level row holds n_scored deciles of 0 .. 10 on domains of that row, NONE and EMPTY hold none; no byte is left unwritten"""
    a = snap.arrays
    for i in range(len(r.q)):
        row, dec = r.score_rows[i], r.deciles[i]
        scored = dec != NO_SCORE
        assert (dec[scored] <= 10).all(), f"{what} query {i}: a decile that is neither <= 10 nor 255"
        if row["level_row"] < 0:
            assert row["level_row"] in (NONE_ROW, EMPTY_ROW) and row["n_scored"] == 0 and not scored.any(), f"{what} query {i}: {row}"
        else:
            assert scored.sum() == row["n_scored"] >= 1 and (a["domain_level"][scored] == row["level_row"]).all(), f"{what} query {i}: {row}"
            want = sorted(int(np.floor((x + 1) / row["n_scored"] * 10)) for x in range(row["n_scored"]))
            assert sorted(dec[scored].tolist()) == want, f"{what} query {i}: the deciles are calculateNodeScores' for {row['n_scored']} domains"


def both_paths_scored(snap, cfg, jobs, what, want_path=WIDE, state=None, sim=None, oracle=True, **kw):
    """the scored call on both paths of one session: against each other byte for byte, against kai_subset_nodes' outputs, "changes nothing", and (root queries over all nodes)
    against the oracle -> (the chip-wide result, the oracle's per-node scores or None per job)"""
    own = sim is None
    sim = sim or Sim(snap, cfg)
    try:
        plain = sim.subset(jobs, scored=False, **kw)
        w, e = sim.subset(jobs, **kw), sim.subset(jobs, engine=True, **kw)
    finally:
        if own: sim.__exit__()
    for r, name in ((w, "chip-wide allowed"), (e, "engine path")):
        assert r.call_status == 0 and r.unchanged == 1, f"{what} ({name}): status {r.call_status}, unchanged {r.unchanged}"
        check_consistent(snap, r.q, r.rows, r.ans, r.sets, r.masks, r.res, f"{what} ({name})")
        check_rows(snap, r, f"{what} ({name})")
    assert w.res.path == want_path and e.res.path == ENGINE, (what, w.res.path, e.res.path)
    assert plain.call_status == 0 and same_answers((w.ans, w.sets, w.masks), (plain.ans, plain.sets, plain.masks)) and w.res.path == plain.res.path, f"{what}: kai_subset_nodes' outputs differ"
    assert (plain.score_rows["level_row"] == -77).all() and (plain.deciles == 0x77).all(), "kai_subset_nodes writes no scores"
    assert same_answers((w.ans, w.sets, w.masks), (e.ans, e.sets, e.masks)), f"{what}: the two paths' sets differ"
    assert w.score_rows.tobytes() == e.score_rows.tobytes() and w.deciles.tobytes() == e.deciles.tobytes(), \
        f"{what}: the two paths' scores differ, first at query {int(np.nonzero((w.score_rows != e.score_rows) | (w.deciles != e.deciles).any(axis=1))[0][0])}"
    refs = []
    if oracle:
        at = state if state is not None else snap
        for i, j in enumerate(jobs):
            ref = oracle_scores(at, cfg, j)
            refs.append(ref)
            if ref is None:
                assert w.ans["status"][i] in (BAD_LEVEL, abi.SUBSET_NO_TOPOLOGY), f"{what} job {j}: the oracle's function returned an error, the call says {w.ans['status'][i]}"
                continue
            got = node_scores(snap, w.score_rows[i], w.deciles[i])
            assert np.array_equal(got, ref), f"{what} job {j}: scores differ from the oracle's at nodes {np.nonzero(got != ref)[0][:8].tolist()}: {got[got != ref][:8]} vs {ref[got != ref][:8]}"
    return w, refs


@pytest.mark.parametrize("i", range(len(KAT.CASES) + 3 + len(KAT.SCENES)))
def test_sim_scores_on_the_references_tables(i):
    name, snap, cfg = kat_scenes()[i]
    both_paths_scored(snap, cfg, [snap.job_names.index("test-job")], name)


def score_scene(racks, n_tasks=1, cpu=1):
    """the scenes of _topology_scores (tests/test_oracle_topology_kat.py): racks {rack: [cores of each node]}, a gang with required zone and preferred rack"""
    nodes = {f"{r}-n{i}": {"CPUMillis": c, "GPUs": 0, "MaxTaskNum": 100, "Labels": {"zone": "zone1", "rack": r}} for r, cs in racks.items() for i, c in enumerate(cs)}
    return KAT._scene(nodes, [{"Name": "test-job", "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": cpu, "RootSubGroupSet": KAT._root("zone", "rack"), "Tasks": [{"State": "Pending"}] * n_tasks}])


@pytest.mark.parametrize("racks,want", [({"rack1": [1, 1]}, {"rack1-n0": 10, "rack1-n1": 10}),
                                        ({"rack3": [1], "rack2": [2], "rack1": [3]}, {"rack1-n0": 10, "rack2-n0": 6, "rack3-n0": 3}),
                                        ({"rack4": [1], "rack3": [2], "rack2": [3], "rack1": [4]}, {"rack1-n0": 10, "rack2-n0": 7, "rack3-n0": 5, "rack4-n0": 2})], ids=["10", "3-6-10", "2-5-7-10"])
def test_sim_scores_of_test_calculate_node_scores(racks, want):
    snap, cfg = score_scene(racks)
    w, refs = both_paths_scored(snap, cfg, [0], str(racks))
    got = node_scores(snap, w.score_rows[0], w.deciles[0])
    assert {snap.node_names[n]: got[n] for n in range(snap.n_nodes)} == {k: v * abi.TOPO_SCORE_UNIT for k, v in want.items()} and refs[0] is not None


@pytest.mark.parametrize("N,zones,racks", SHAPES)
def test_sim_scores_synthetic_against_the_oracle(N, zones, racks):
    snap, cfg = synthetic(N, zones, racks)
    jobs = topology_jobs(snap)
    a = snap.arrays
    pref = [j for j in jobs if a["group_preferred_level"][a["job_root_group"][j]] >= 0]
    refs = {j: oracle_scores(snap, cfg, j) for j in pref}
    have = [j for j in pref if refs[j] is not None and (refs[j] >= 0).any()]
    # what makes the comparison worth making, from the oracle alone
    if (N, zones, racks) == (70, 2, 3):
        assert len(pref) == 9 and sum(len(set(refs[j][refs[j] >= 0].tolist())) > 1 for j in have) == 3, "9 preferred-level gangs, 3 of them with more than one distinct score"
    else:
        assert len(have) == 5, "5 preferred-level gangs with scores"
        for j in have:
            assert {int(v // abi.TOPO_SCORE_UNIT) for v in refs[j][refs[j] >= 0]} == set(range(11)) and (refs[j] < 0).any(), "every decile 0 .. 10 and unscored (unlabelled) nodes in every row"
    w, _ = both_paths_scored(snap, cfg, jobs, f"N {N}")
    kinds = set(w.score_rows["level_row"].tolist())
    assert NONE_ROW in kinds and max(kinds) >= 0
    if N == 70:  # other workgroup shapes and a grid below the queries: the same scores
        with Sim(snap, cfg) as sim:
            for lanes, wgs in ((100, 3), (64, 1), (1, 1 << 20)):
                r = sim.subset(jobs, lanes=lanes, wgs=wgs)
                assert r.score_rows.tobytes() == w.score_rows.tobytes() and r.deciles.tobytes() == w.deciles.tobytes(), (lanes, wgs)


def test_sim_scores_of_levels_the_topology_does_not_have():
    """a preferred level the topology does not have: EMPTY; a required level it does not have with a preferred level it has: BAD_LEVEL with scores"""
    snap, cfg = synthetic(70, 2, 3)
    a = snap.arrays
    jobs = topology_jobs(snap)
    with Sim(snap, cfg) as sim:
        base = sim.subset(jobs)
    scored = [i for i in range(len(jobs)) if base.score_rows["level_row"][i] >= 0 and base.ans["status"][i] == OK]
    assert len(scored) >= 2
    g0, g1 = (int(a["job_root_group"][jobs[i]]) for i in scored[:2])
    a["group_preferred_level"][g0] = 7
    a["group_required_level"][g1] = 6
    snap.finalize()
    w, _ = both_paths_scored(snap, cfg, jobs, "levels the topology does not have", oracle=False)
    i0, i1 = scored[:2]
    assert w.ans["status"][i0] == BAD_LEVEL and tuple(w.score_rows[i0]) == (EMPTY_ROW, 0)
    assert w.ans["status"][i1] == BAD_LEVEL and w.score_rows["level_row"][i1] >= 0 and w.deciles[i1].tobytes() == base.deciles[i1].tobytes(), "the scores are recorded in front of the level checks"


# ---------------------------------------------------------------------------------------------- three levels
def three_level_scene():
    """zone / block / rack over 96 nodes (2 x 3 x 4 x 4), six of them without labels; nodes of different sizes and a few running pods, so that the ratios differ; gangs with a
    required zone and a preferred block or rack, one without a required level, one with a required block, one no zone can take"""
    topo = [{"ObjectMeta": {"Name": "test-topology"}, "Spec": {"Levels": [{"NodeLabel": "zone"}, {"NodeLabel": "block"}, {"NodeLabel": "rack"}]}}]
    nodes = {}
    for n in range(96):
        z, b, r = n // 48, n // 16, n // 4
        labels = {} if n % 17 == 5 else {"zone": f"zone{z}", "block": f"block{b:02d}", "rack": f"rack{r:02d}"}
        nodes[f"node{n:03d}"] = {"CPUMillis": 8 + (n * 7) % 13, "GPUs": 0, "MaxTaskNum": 100, "Labels": labels}
    root = lambda req, pref: {"Name": "", "PodSets": [], "SubGroups": [], "TopologyConstraint": {"Topology": "test-topology", "RequiredLevel": req, "PreferredLevel": pref}}
    gang = lambda name, req, pref, n: {"Name": name, "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": 1, "RootSubGroupSet": root(req, pref), "Tasks": [{"State": "Pending"}] * n}
    jobs = [gang("zone-block", "zone", "block", 4), gang("zone-rack", "zone", "rack", 4), gang("none-rack", "", "rack", 30), gang("block-rack", "block", "rack", 3), gang("too-large", "zone", "block", 2000),
            {"Name": "running", "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": 3, "Tasks": [{"State": "Running", "NodeName": f"node{n:03d}"} for n in (0, 1, 9, 20, 21, 22, 50, 70, 71, 90)]}]
    return KAT._scene(nodes, jobs, topo)


def test_sim_three_levels():
    snap, cfg = three_level_scene()
    a = snap.arrays
    assert a["node_domain"].shape[0] == 3 and (a["node_domain"][0] < 0).sum() == 6
    jobs = [snap.job_names.index(x) for x in ("zone-block", "zone-rack", "none-rack", "block-rack", "too-large")]
    w, refs = both_paths_scored(snap, cfg, jobs, "three levels")
    assert [int(x) for x in w.score_rows["level_row"]] == [1, 2, 2, 2, NONE_ROW] and [int(x) for x in w.score_rows["n_scored"][:4]] == [6, 24, 24, 24]
    assert all(r is not None for r in refs) and len(set(refs[1][refs[1] >= 0].tolist())) == 11, "rack scores take every decile"
    # parent rows: zone 0 (the common domain is the zone: its 3 blocks / 12 racks), block 1 (preferred block: the common domain is at the preferred level itself, one domain,
    # decile 10; preferred rack: its 4 racks)
    zone0, block1 = a["node_domain"][0] == a["node_domain"][0][0], a["node_domain"][1] == a["node_domain"][1][16]
    q_jobs = [jobs[0], jobs[1], jobs[0], jobs[1]]
    r, _ = both_paths_scored(snap, cfg, q_jobs, "three levels, parent rows", oracle=False, rows=[zone0, block1], nodeset_of=[0, 0, 1, 1])
    assert [tuple(x) for x in r.score_rows] == [(1, 3), (2, 12), (1, 1), (2, 4)]
    assert r.deciles[2][r.deciles[2] != NO_SCORE].tolist() == [10] and np.nonzero(r.deciles[2] != NO_SCORE)[0][0] == a["node_domain"][1][16]
    # a sub-tree's ranking is the whole tree's order restricted to it
    for sub, full in ((r.deciles[1], w.deciles[1]), (r.deciles[3], w.deciles[1])):
        doms = np.nonzero(sub != NO_SCORE)[0]
        assert [int(d) for d in doms[np.argsort(sub[doms], kind="stable")]] == [int(d) for d in doms[np.argsort(full[doms], kind="stable")]] or len(set(full[doms].tolist())) < len(doms)


# ---------------------------------------------------------------------------------------------- sub-groups and parent rows
@pytest.mark.parametrize("seed", [7, 6])
def test_sim_sub_groups_and_parent_rows(seed):
    """replica_scene() (seed 7: no root sub-group set with a preferred zone fits, every row is NONE) and seed 6, where three such roots have scores"""
    snap, cfg = replica_scene(seed)
    a = snap.arrays
    with Sim(snap, cfg) as sim:
        roots, _ = both_paths_scored(snap, cfg, np.arange(snap.n_jobs, dtype=np.int32), "replica roots", sim=sim)
        assert (roots.score_rows["level_row"] == NONE_ROW).any() and (roots.score_rows["level_row"] >= 0).sum() == (3 if seed == 6 else 0), "root sub-group sets with a preferred zone that fit have scores"
        mk = lambda engine: (lambda jobs, groups, podsets, rows, ns: (lambda r: (r.ans, r.sets, r.masks, r))(sim.subset(jobs, groups, podsets, rows, ns, engine=engine)))
        rw, re = inner_walk(mk(False), snap), inner_walk(mk(True), snap)
    assert len(rw) == len(re) == 3
    seen = set()
    for (q, rows, w), (_q, _rows, e) in zip(rw, re):
        assert w[3].call_status == 0 and e[3].call_status == 0 and w[3].unchanged and e[3].unchanged and w[3].res.path == WIDE and e[3].res.path == ENGINE
        assert same_answers(w, e) and w[3].score_rows.tobytes() == e[3].score_rows.tobytes() and w[3].deciles.tobytes() == e[3].deciles.tobytes(), "the two paths on the inner queries"
        check_rows(snap, w[3], "inner")
        for i in range(len(q)):
            g, s = int(q["group"][i]), int(q["podset"][i])
            grp = int(a["job_root_group"][q["job"][i]]) if g < 0 and s < 0 else g
            topo, pref = (a["podset_topology"][s], a["podset_preferred_level"][s]) if s >= 0 else (a["group_topology"][grp], a["group_preferred_level"][grp])
            # the reference returns before line 88 where there is no constraint or no task or where the common domain does not fit; without a preferred level it records
            # nothing.  An answer OK or BAD_LEVEL is behind the common domain's fit; NO_FIT does not say which of its two checks failed (there the two paths agree, above)
            has = w[3].score_rows["level_row"][i] != NONE_ROW
            if topo < 0 or pref < 0 or w[0]["tasks"][i] == 0: assert not has, (q[i], w[0][i], w[3].score_rows[i])
            elif w[0]["status"][i] in (OK, BAD_LEVEL): assert has, (q[i], w[0][i], w[3].score_rows[i])
            seen.add((bool(has), int(w[0]["status"][i])))
    # (the fixtures' child SubGroupSets and pod-sets carry a required level only: their rows are NONE, and their tasks are scored with the root's row, the nearest ancestor's)
    if seed == 7: assert (False, OK) in seen and (False, NO_FIT) in seen, "inner queries that list sets and inner queries that list none occur"


# ---------------------------------------------------------------------------------------------- the session is as it was
def test_sim_the_next_allocate_is_the_twins():
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    with Sim(snap, cfg) as twin:
        twin.action("allocate"); t_st, t_nd, t_ops = twin.state()
    for engine in (False, True):
        with Sim(snap, cfg) as sim:
            r = sim.subset(jobs, engine=engine)
            assert r.call_status == 0 and r.unchanged == 1
            sim.action("allocate"); st, nd, ops = sim.state()
        assert ops.tobytes() == t_ops.tobytes() and len(ops) > 0 and np.array_equal(st, t_st) and np.array_equal(nd, t_nd)


def test_sim_a_state_only_an_action_reaches():
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    with Sim(snap, cfg) as sim:
        sim.action("allocate"); st, nd, _ = sim.state()
        after = abi.apply_delta(snap, np.arange(snap.n_pods), st, nd)
        both_paths_scored(snap, cfg, jobs, "after allocate", state=after, sim=sim)


def test_sim_sessions_the_chip_wide_path_does_not_take():
    snap, cfg = synthetic(70, 2, 3)
    T.pkg.synth.add_fractions(snap, 7, frac=0.3)
    w, refs = both_paths_scored(snap, cfg, topology_jobs(snap), "fractions", want_path=ENGINE)
    assert any(r is not None and (r >= 0).any() for r in refs)


# ---------------------------------------------------------------------------------------------- scored lists
def scored_case(N, zones, racks, n_pods=12, releasing=False):
    """the synthetic scene, its root score rows, and list queries: pods of the preferred-level gangs over the row of their zone set (or all nodes), with the gang's row, an
    all-NONE row and scores = -1"""
    snap, cfg = synthetic(N, zones, racks)
    a = snap.arrays
    if releasing:
        run = np.nonzero(a["pod_status"] == abi.POD_STATUS["Running"])[0]
        a["pod_status"][run[::7]] = abi.POD_STATUS["Releasing"]
        snap.finalize()
    return snap, cfg


def list_queries(snap, r, jobs, n_pods=12):
    """(pods, nodeset_of, rows, scores_of): for every query of r with a level row, the job's first pending pods over its first node set and over all nodes"""
    a = snap.arrays
    pods, ns, rows, so = [], [], [], []
    for i, j in enumerate(jobs):
        if r.score_rows["level_row"][i] < 0: continue
        mine = np.nonzero((a["pod_job"] == j) & (a["pod_status"] == abi.POD_STATUS["Pending"]))[0][:2]
        for p in mine:
            if r.ans["n_sets"][i] > 0:
                rows.append(r.masks[r.ans["first"][i] + r.ans["n_sets"][i] - 1]); pods.append(int(p)); ns.append(len(rows) - 1); so.append(i)
            pods.append(int(p)); ns.append(-1); so.append(i)
        if len(pods) >= n_pods: break
    return pods, ns, rows, so


def check_scored_lists(snap, r, pods, ns, rows, so, scored, unscored_full, k, what=""):
    """the properties of a scored list against the unscored full list over the same node set: scored nodes only, non-increasing in decile, inside one decile the unscored
    list's relative order, n_out = min(k, scored nodes of the unscored list)"""
    a = snap.arrays
    for x in range(len(pods)):
        row, dec = r.score_rows[so[x]], r.deciles[so[x]]
        dd = a["node_domain"][int(row["level_row"])]
        dn = lambda n: int(dec[dd[n]]) if dd[n] >= 0 else NO_SCORE
        got, full = [n for n, _ in scored[x]], [n for n, _ in unscored_full[x]]
        assert all(dn(n) != NO_SCORE for n in got), f"{what} query {x}: a listed node has no score"
        ds = [dn(n) for n in got]
        assert ds == sorted(ds, reverse=True), f"{what} query {x}: the list is not non-increasing in decile"
        keep = [n for n in full if dn(n) != NO_SCORE]
        if len(full) < 64:  # (the unscored list is complete: every node that fits is in it)
            assert len(got) == min(k, len(keep)), f"{what} query {x}: n_out {len(got)}, {len(keep)} nodes of the unscored list carry a score"
            want = sorted(keep, key=lambda n: -dn(n))[:k]  # (stable: the unscored list's order inside a decile)
            assert got == want, f"{what} query {x}: {got} vs {want}"
            assert dict(scored[x]) == {n: p for n, p in unscored_full[x] if n in set(got)}, f"{what} query {x}: is_pipeline differs from the unscored list's"
        else:
            for d in set(ds):
                part = [n for n in got if dn(n) == d]
                inter = [n for n in full if n in set(part)]
                assert [n for n in part if n in set(full)] == inter, f"{what} query {x}: the order inside decile {d}"


@pytest.mark.parametrize("N,zones,racks", [(70, 2, 3), (300, 3, 5)])
def test_sim_scored_lists(N, zones, racks):
    snap, cfg = scored_case(N, zones, racks)
    jobs = topology_jobs(snap)
    with Sim(snap, cfg) as sim:
        r = sim.subset(jobs)
        pods, ns, rows, so = list_queries(snap, r, jobs)
        assert len(pods) >= 8 and any(x >= 0 for x in ns) and any(x < 0 for x in ns)
        full = sim.ordered(pods, 64, rows, ns, scored=False)
        assert any(0 < len(l) < 64 for l in full), "a complete unscored list occurs"
        none_rows = np.zeros(len(r.score_rows), R_DT); none_rows["level_row"] = NONE_ROW
        empty_rows = np.zeros(len(r.score_rows), R_DT); empty_rows["level_row"] = EMPTY_ROW
        changed = False
        for k in (1, 8, 64):
            ref = [l[:k] for l in full]
            for lanes, grid in ((256, 1 << 20), (64, 1 << 20), (256, 3)):
                got = sim.ordered(pods, k, rows, ns, r.score_rows, r.deciles, so, lanes=lanes, grid=grid)
                check_scored_lists(snap, r, pods, ns, rows, so, got, full, k, f"k {k} lanes {lanes} grid {grid}")
                changed |= any(g and u and g[0] != u[0] for g, u in zip(got, ref))
                assert sim.ordered(pods, k, rows, ns, none_rows, r.deciles, so, lanes=lanes, grid=grid) == ref, "rows of NONE reproduce kai_ordered_nodes' lists"
                assert sim.ordered(pods, k, rows, ns, r.score_rows, r.deciles, None, lanes=lanes, grid=grid) == ref, "scores = -1 reproduces kai_ordered_nodes' lists"
            assert all(l == [] for l in sim.ordered(pods, k, rows, ns, empty_rows, r.deciles, so)), "an EMPTY row gives n_out = 0"
        assert changed, "the scores change the head of some list"


REVERSED = r'''
import json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import test_topo_scores as tt
snap, cfg = tt.scored_case(70, 2, 3)
jobs = tt.topology_jobs(snap)
with tt.Sim(snap, cfg) as sim:
    r = sim.subset(jobs)
    pods, ns, rows, so = tt.list_queries(snap, r, jobs)
    print(json.dumps([r.score_rows.tobytes().hex(), r.deciles.tobytes().hex(), {str(k): sim.ordered(pods, k, rows, ns, r.score_rows, r.deciles, so) for k in (1, 8, 64)}]))
'''


def test_kernel_bodies_with_the_wave_order_reversed():
    """the emulator's waves take their turns in reverse (KW_EMU_ORDER=1, read once per process: a fresh one): the same scores and the same lists"""
    snap, cfg = scored_case(70, 2, 3)
    jobs = topology_jobs(snap)
    with Sim(snap, cfg) as sim:
        r = sim.subset(jobs)
        pods, ns, rows, so = list_queries(snap, r, jobs)
        want = {str(k): [[list(e) for e in l] for l in sim.ordered(pods, k, rows, ns, r.score_rows, r.deciles, so)] for k in (1, 8, 64)}
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + REVERSED], env=dict(os.environ, KW_EMU_ORDER="1"), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got == [r.score_rows.tobytes().hex(), r.deciles.tobytes().hex(), want]


# ---------------------------------------------------------------------------------------------- a gang placed by queries lands where the allocate action puts it
def gang_scene():
    """one zone, three racks of two 4-GPU nodes; running pods use 2 GPUs of rack1, 4 of rack2 and none of rack3; a pending gang of six 2-GPU pods with required zone and
    preferred rack.  No rack has 12 free GPUs, so the zone is the only set and the scores alone decide which rack fills first; the configuration bin-packs."""
    nodes = {f"{r}-n{i}": {"CPUMillis": 64000, "GPUs": 4, "MaxTaskNum": 100, "Labels": {"zone": "zone1", "rack": r}} for r in ("rack1", "rack2", "rack3") for i in range(2)}
    run = lambda name, node, g: {"Name": name, "Priority": 50, "QueueName": "q", "RequiredGPUsPerTask": g, "Tasks": [{"State": "Running", "NodeName": node}]}
    jobs = [{"Name": "gang", "Priority": 50, "QueueName": "q", "RequiredGPUsPerTask": 2, "RootSubGroupSet": KAT._root("zone", "rack"), "Tasks": [{"State": "Pending"}] * 6},
            run("r1", "rack1-n0", 2), run("r2a", "rack2-n0", 2), run("r2b", "rack2-n1", 2)]
    case = {"Name": "scene", "Nodes": nodes, "Topologies": KAT.TOPO, "Queues": [{"Name": "q", "DeservedGPUs": 24}], "Jobs": jobs, "JobExpectedResults": {}}
    snap, cfg, _ = T.case_to_snapshot(case)
    cfg.plugins |= abi.PLUGINS["topology"]
    assert cfg.gpu_strategy == abi.BINPACK
    return snap, cfg


def walk_the_gang(snap, cfg, ref, subset, ordered, unscored, apply):
    """the walk of the issue's item 8 over callables of a session -> the first unscored node"""
    gang = snap.job_names.index("gang")
    r_ans, r_masks, score_rows, deciles = subset([gang])
    assert r_ans["status"][0] == OK and r_ans["n_sets"][0] == 1 and r_masks[0].all(), "no rack can take the gang: the zone is the only set"
    assert score_rows["level_row"][0] == 1 and sorted(deciles[0][deciles[0] != NO_SCORE].tolist()) == [3, 6, 10]
    mine = [(k, p, n, j) for k, p, n, j in ref.ops if j == gang]
    assert len(mine) == 6 and all(k == 0 for k, _, _, _ in mine), "the oracle allocates the whole gang"
    first_unscored = None
    for stmt, (kind, pod, node, job) in enumerate(mine):
        got = ordered([pod], 1, [r_masks[0]], [0], score_rows, deciles, [0])
        if first_unscored is None: first_unscored = unscored([pod], 1, [r_masks[0]], [0])[0][0][0]
        assert got[0] and got[0][0][0] == node, f"pod {pod}: the scored list's head is {snap.node_names[got[0][0][0]] if got[0] else None}, the oracle puts it on {snap.node_names[node]}"
        op = np.zeros(1, T.pkg.core._OP_DTYPE); op["kind"], op["pod"], op["node"], op["job"], op["stmt"] = kind, pod, node, job, 0
        apply(op)
    return first_unscored, mine


def test_sim_a_gang_placed_by_queries_lands_where_the_allocate_action_puts_it():
    snap, cfg = gang_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    with Sim(snap, cfg) as sim:
        def subset(jobs):
            r = sim.subset(jobs)
            e = sim.subset(jobs, engine=True)
            assert r.call_status == 0 and e.call_status == 0 and r.score_rows.tobytes() == e.score_rows.tobytes() and r.deciles.tobytes() == e.deciles.tobytes()
            return r.ans, r.masks, r.score_rows, r.deciles
        first_unscored, mine = walk_the_gang(snap, cfg, ref, subset, lambda *a: sim.ordered(*a), lambda *a: sim.ordered(*a[:4], scored=False), sim.apply)
        st, nd, _ = sim.state()
    assert first_unscored != mine[0][2], "the unscored kai_ordered_nodes puts the first pod elsewhere: the gap the scored call closes"
    assert snap.node_names[mine[0][2]].startswith("rack3") and not snap.node_names[first_unscored].startswith("rack3"), "the scores send the gang to the emptiest rack, bin-packing alone to a node in use"
    with Sim(snap, cfg) as twin:
        twin.action("allocate"); t_st, t_nd, _ = twin.state()
    assert np.array_equal(st, t_st) and np.array_equal(nd, t_nd) and np.array_equal(st, ref.pod_status) and np.array_equal(nd, ref.pod_node)


# ---------------------------------------------------------------------------------------------- the stand-alone program
def test_stand_alone_program(tmp_path):
    """the fixed case behind -DKAI_TSSIM_MAIN builds and passes, with the emulator's waves in both orders"""
    exe = str(tmp_path / "topo_scores_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKAI_TSSIM_MAIN", "-o", exe, SIM_SRC])
    for order in ("0", "1"):
        r = subprocess.run([exe], env=dict(os.environ, KW_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "topo_scores_sim: ok" in r.stdout, (order, r.stdout[-2000:], r.stderr[-2000:])


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan (a program of its own: nothing is loaded into python)"""
    exe = str(tmp_path / "topo_scores_sim_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKAI_TSSIM_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0"), capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "topo_scores_sim: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
