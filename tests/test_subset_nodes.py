"""kai_subset_nodes without a GPU.

 - the export, the ABI structs and constants, the header text;
 - arguments under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp, as tests/test_ordered_nodes.py does): every refusal is
   made before the first device call and leaves the device memory image, the session and the caller's arrays as they were; n_queries == 0 is KAI_OK without a device call;
 - the kernel bodies and the call's control flow (kai_subset_nodes.hpp: sn_count and the emit, both paths) run with emulated lanes by tests/host_sim/subset_nodes_sim.cpp on a
   session of the host simulation, against the oracle's subSetNodesFn (kai_oracle_subset_nodes_all, kai_oracle_subset_nodes, kai_oracle_tree_allocatable) on the snapshot
   that equals the session's state: the reference's own tables (tests/test_oracle_topology_kat.py), synthetic topologies with unlabelled nodes, and the sub-group walk of
   the replica fixtures.  The capacity protocol ("the count needed, nothing written") is part of the stand-alone program's fixed case.
The simulation is loaded as a library, as tests/test_job_order.py loads its own (a snapshot has no file form a program could read); the stand-alone program is the fixed case
behind -DKAI_SNSIM_MAIN, which is also what runs under the sanitizers.  The parity claim on the device is tests/test_gpu_subset_nodes.py."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
synth = T.pkg.synth
NONE, WIDE, ENGINE = abi.SUBSET_PATH_NONE, abi.SUBSET_PATH_WIDE, abi.SUBSET_PATH_ENGINE
OK, NO_TOPOLOGY, NO_FIT, BAD_LEVEL = abi.SUBSET_OK, abi.SUBSET_NO_TOPOLOGY, abi.SUBSET_NO_FIT, abi.SUBSET_BAD_LEVEL
Q_DT = np.dtype([("job", "<i4"), ("group", "<i4"), ("podset", "<i4"), ("nodeset", "<i4")])
A_DT = np.dtype([("status", "<i4"), ("n_sets", "<i4"), ("first", "<i4"), ("tasks", "<i4"), ("common_domain", "<i4"), ("pad", "<i4")])
S_DT = np.dtype([("domain", "<i4"), ("level", "<i4"), ("allocatable_pods", "<i4"), ("n_nodes", "<i4")])


def test_exports_and_struct_sizes():
    assert "kai_subset_nodes" in T.pkg.core.EXPORTS
    assert [C.sizeof(x) for x in (abi.KaiSubsetParams, abi.KaiSubsetQuery, abi.KaiSubsetAnswer, abi.KaiNodeSet, abi.KaiSubsetResult)] == [8, 16, 24, 16, 16]
    assert [f[0] for f in abi.KaiSubsetAnswer._fields_] == list(A_DT.names) and [f[0] for f in abi.KaiNodeSet._fields_] == list(S_DT.names) and [f[0] for f in abi.KaiSubsetQuery._fields_] == list(Q_DT.names)
    assert (abi.SUBSET_VERSION, abi.SUBSET_ENGINE_PATH, NONE, WIDE, ENGINE, abi.SUBSET_PARENT, abi.subset_root(0), abi.subset_root(3)) == (1, 1, 0, 1, 2, -1, -2, -5)
    assert (OK, NO_TOPOLOGY, NO_FIT, BAD_LEVEL) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    for text in ("#define KAI_SUBSET_VERSION 1u", "#define KAI_SUBSET_ENGINE_PATH 0x1u", "#define KAI_SUBSET_PATH_WIDE 1", "#define KAI_SUBSET_PATH_ENGINE 2", "#define KAI_SUBSET_PARENT (-1)",
                 "#define KAI_SUBSET_ROOT(t) (-2 - (t))", "KAI_SUBSET_NO_TOPOLOGY = 1", "KAI_SUBSET_NO_FIT = 2", "KAI_SUBSET_BAD_LEVEL = 3",
                 "typedef struct kai_subset_query  { int32_t job; int32_t group; int32_t podset; int32_t nodeset; } kai_subset_query;",
                 "typedef struct kai_node_set      { int32_t domain; int32_t level; int32_t allocatable_pods; int32_t n_nodes; } kai_node_set;",
                 "int kai_subset_nodes(kai_core* core, const kai_subset_params* params,", "plugins/topology/job_filtering.go:34-112", "calculateNodeScores"):
        assert text in hdr, text
    assert hasattr(T.pkg.load_library(), "kai_subset_nodes") and hasattr(T.pkg.core.Session, "subset_nodes")


# ---------------------------------------------------------------------------------------------- scenes
def topo_cfg(cfg=None):
    cfg = cfg or abi.default_config()
    cfg.plugins |= abi.PLUGINS["topology"]
    return cfg


def kat_scenes():
    """every scene of tests/test_oracle_topology_kat.py as (name, snapshot, config): its CASES, the pods that already run, releasing resources, a job that requests nothing,
    the ratio order of racks (the _node_sets racks), and SCENES"""
    out = []
    for line, name, cpu, tasks, tc, nodes, _want in KAT.CASES:
        root = {"Name": "", "PodSets": [], "SubGroups": [], "TopologyConstraint": {"Topology": tc[0], "RequiredLevel": tc[1], "PreferredLevel": tc[2]} if tc else None}
        case = {"Name": name, "Nodes": nodes, "Topologies": KAT.TOPO, "Queues": [{"Name": "q", "DeservedGPUs": 1}],
                "Jobs": [{"Name": "test-job", "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": cpu, "RootSubGroupSet": root,
                          "Tasks": [{"State": "Pending", **({"RequiredGPUs": g} if g is not None else {})} for g in tasks]}], "JobExpectedResults": {}}
        snap, cfg, _ = T.case_to_snapshot(case)
        out.append((f"{line}:{name}", snap, topo_cfg(cfg)))
    topo1 = [{"ObjectMeta": {"Name": "test-topology"}, "Spec": {"Levels": [{"NodeLabel": "zone"}]}}]
    nodes = {"node1": {"CPUMillis": 2, "GPUs": 0, "MaxTaskNum": 100, "Labels": {"zone": "zone1"}}, "node2": {"CPUMillis": 3, "GPUs": 0, "MaxTaskNum": 100, "Labels": {"zone": "zone2"}}}
    root = {"Name": "", "PodSets": [{"Name": "default", "MinAvailable": 2, "TopologyConstraint": None}], "SubGroups": [], "TopologyConstraint": {"Topology": "test-topology", "RequiredLevel": "zone", "PreferredLevel": ""}}
    out.append(("the pods that already run", *KAT._scene(nodes, [{"Name": "test-job", "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": 1, "RootSubGroupSet": root,
                                                                 "Tasks": [{"State": "Running", "NodeName": "node2"}, {"State": "Pending"}, {"State": "Pending"}]}], topo1)))
    for racks, cpu, gpus in (({"rack3": (100, 5), "rack1": (100, 2), "rack2": (100, 8)}, 0.001, 1), ({"rack3": (5, 0), "rack1": (2, 0), "rack2": (8, 0)}, 1, 0)):
        nodes = {f"node-{r}": {"CPUMillis": c, "GPUs": g, "MaxTaskNum": 100, "Labels": {"zone": "zone1", "rack": r}} for r, (c, g) in racks.items()}
        out.append((f"ratio order of racks, gpus {gpus}", *KAT._scene(nodes, [{"Name": "test-job", "Priority": 50, "QueueName": "q", "RequiredCPUsPerTask": cpu, "RequiredGPUsPerTask": gpus,
                                                                             "RootSubGroupSet": KAT._root("zone", "rack"), "Tasks": [{"State": "Pending"}]}])))
    for name in sorted(KAT.SCENES):
        out.append((name, *KAT.SCENES[name]()))
    return out


def synthetic(N, zones, racks_per_zone, seed=5, unlabelled=True):
    """make_crowded_snapshot + add_topology, a tenth of the nodes outside the topology, one topology job whose constraint names a topology that does not exist and one
    whose required level the topology does not have"""
    snap = synth.make_crowded_snapshot(N, seed, n_pending_jobs=40)
    synth.add_topology(snap, seed, zones, racks_per_zone, req_rack_frac=0.5, pref_rack_frac=0.4)
    a = snap.arrays
    if unlabelled:
        a["node_domain"] = a["node_domain"].copy(); a["node_domain"][:, np.random.default_rng(1).random(N) < 0.1] = -1
    tj = np.nonzero(a["group_topology"] == 0)[0]
    assert len(tj) >= 6
    a["group_topology"][tj[-1]] = -2
    snap.finalize()
    cfg = topo_cfg()
    fits = [g for g in tj[:-1] if oracle_answer(snap, cfg, int(a["group_job"][g]))[0] == OK]  # (a gang whose common domain has room: the level check is reached)
    assert len(fits) >= 2
    a["group_required_level"][fits[-1]] = 5
    snap.finalize()
    return snap, cfg


def replica_scene(seed=7):
    """the sub-group fixtures of tests/test_gpu_parity.py:413-415"""
    snap = synth.make_crowded_snapshot(6 + seed % 13, 3000 + seed, fill=0.8 + 0.1 * (seed % 2), queue_levels=((2, 2), (3,), (2, 2, 2))[seed % 3], two_podsets_frac=0.6, n_pending_jobs=14)
    synth.add_replica_topology(snap, seed, zones=2, nodes_per_rack=2 + seed % 2)
    return snap, topo_cfg(abi.default_config(max_consolidation_preemptees=-1))


def topology_jobs(snap):
    """the jobs whose root group carries a constraint (a topology, or the -2 of a missing one)"""
    a = snap.arrays
    if "group_topology" not in a or snap.n_jobs == 0: return np.arange(snap.n_jobs, dtype=np.int32)
    return np.nonzero(a["group_topology"][a["job_root_group"]] != -1)[0].astype(np.int32)


# ---------------------------------------------------------------------------------------------- the oracle's side
def oracle_answer(snap, cfg, job):
    """(status, [sorted node tuple per node set, in order]) of subSetNodesFn for the job's root sub-group set over all nodes, on a freshly loaded session of `snap`"""
    lib = T.Oracle.lib(); lib.kai_oracle_subset_nodes_all.restype = C.c_int; lib.kai_oracle_subset_nodes.restype = C.c_int
    s = snap.as_struct(); N = snap.n_nodes
    D = len(snap.arrays["domain_parent"]) if "domain_parent" in snap.arrays else 0
    cap = (D + 4) * (N + 1) + 8
    out = np.zeros(cap, np.int32); n_sets = C.c_int(0); first = np.zeros(max(N, 1), np.int32)
    rc = lib.kai_oracle_subset_nodes(C.byref(cfg), C.byref(s), int(job), first.ctypes.data_as(C.POINTER(C.c_int32)), N, C.byref(n_sets))
    if rc == -1: return BAD_LEVEL, []
    if rc == -2:
        a = snap.arrays
        missing = "group_topology" in a and a["group_topology"][a["job_root_group"][job]] == -2
        return (NO_TOPOLOGY if missing else NO_FIT), []
    n = lib.kai_oracle_subset_nodes_all(C.byref(cfg), C.byref(s), int(job), out.ctypes.data_as(C.POINTER(C.c_int32)), cap)
    assert n > 0, n
    sets, cur = [], []
    for v in out[:n].tolist():
        if v < 0: sets.append(tuple(sorted(cur))); cur = []
        else: cur.append(v)
    assert len(sets) == n_sets.value
    return OK, sets


def oracle_tree_pods(snap, cfg, job):
    """{sorted node tuple of a domain: the set of AllocatablePods the oracle left in domains with those nodes}"""
    lib = T.Oracle.lib(); lib.kai_oracle_tree_allocatable.restype = C.c_int
    N = snap.n_nodes; D = len(snap.arrays["domain_parent"]) + 4
    pods = np.zeros(D, np.int32); member = np.zeros(D * N, np.uint8); s = snap.as_struct()
    nd = lib.kai_oracle_tree_allocatable(C.byref(cfg), C.byref(s), int(job), pods.ctypes.data_as(C.POINTER(C.c_int32)), member.ctypes.data_as(C.POINTER(C.c_uint8)), D)
    assert nd > 0, nd
    got = {}
    for d in range(nd):
        got.setdefault(tuple(np.nonzero(member[d * N:(d + 1) * N])[0].tolist()), set()).add(int(pods[d]))
    return got


def state_snapshot(snap, status, node):
    """the snapshot that equals a session's state: the original with the read-back written into pod_status / pod_node"""
    return abi.apply_delta(snap, np.arange(snap.n_pods), status, node)


def check_consistent(snap, q, rows, ans, sets, masks, res, what=""):
    """what holds of every answer: `first` is the running sum, status OK exactly where there is a set, a set's row holds n_nodes nodes, all of the parent row and of the set's domain"""
    a = snap.arrays
    assert (ans["pad"] == 0).all() and (ans["n_sets"] >= 0).all(), what
    assert np.array_equal(ans["first"], np.concatenate([[0], np.cumsum(ans["n_sets"])[:-1]])), f"{what}: first is the running sum of n_sets"
    assert int(ans["n_sets"].sum()) == len(sets) == res.n_sets and res.pad == 0, what
    assert np.array_equal(ans["status"] == OK, ans["n_sets"] > 0), f"{what}: status OK exactly where a set is listed"
    if masks is None: return
    assert np.array_equal(masks.sum(axis=1), sets["n_nodes"]), f"{what}: n_nodes is the size of the set"
    for i in range(len(q)):
        parent = np.ones(snap.n_nodes, bool) if q["nodeset"][i] < 0 else rows[q["nodeset"][i]]
        for k in range(ans["first"][i], ans["first"][i] + ans["n_sets"][i]):
            d, m = int(sets["domain"][k]), masks[k]
            assert not (m & ~parent).any(), f"{what}: a set leaves the parent row"
            if d == abi.SUBSET_PARENT:
                assert np.array_equal(m, parent) and sets["level"][k] == -1 and sets["allocatable_pods"][k] == -1
            elif d >= 0:
                lvl = int(a["domain_level"][d]) - int(a["topo_level_off"][0])  # (the scenes have one topology)
                assert sets["level"][k] == lvl and np.array_equal(m, parent & (a["node_domain"][a["domain_level"][d]] == d)), f"{what}: the set of domain {d}"
            else:
                assert sets["level"][k] == -1 and np.array_equal(m, parent & (a["node_domain"][0] >= 0)), f"{what}: a root domain's set"


def check_against_oracle(snap_at_state, cfg, jobs, ans, sets, masks, what="", pods=False):
    """root queries over all nodes, one per job of `jobs` in order, against the oracle on the snapshot that equals the session's state -> the oracle's answers"""
    refs = []
    for i, j in enumerate(jobs):
        status, want = oracle_answer(snap_at_state, cfg, j)
        refs.append((status, want))
        assert ans["status"][i] == status, f"{what} job {j}: status {ans['status'][i]}, the oracle has {status}"
        assert ans["n_sets"][i] == len(want), f"{what} job {j}: {ans['n_sets'][i]} sets, the oracle has {len(want)}"
        got = [tuple(np.nonzero(masks[k])[0].tolist()) for k in range(ans["first"][i], ans["first"][i] + ans["n_sets"][i])]
        assert got == want, f"{what} job {j}: node sets differ from the oracle's, first at {[x != y for x, y in zip(got, want)].index(True)}"
        if pods and status == OK and sets["domain"][ans["first"][i]] != abi.SUBSET_PARENT:
            tree = oracle_tree_pods(snap_at_state, cfg, j)
            for k in range(ans["first"][i], ans["first"][i] + ans["n_sets"][i]):
                assert int(sets["allocatable_pods"][k]) in tree[got[k - ans["first"][i]]], f"{what} job {j} set {k}: AllocatablePods {sets['allocatable_pods'][k]}, the oracle has {tree[got[k - ans['first'][i]]]}"
    return refs


def same_answers(x, y):
    """record for record, bitmap word for word (x, y: (ans, sets, masks, ...))"""
    return x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and ((x[2] is None and y[2] is None) or np.array_equal(x[2], y[2]))


def inner_walk(call, snap, max_rows=3):
    """the sub-group walk the action makes: root queries of every job with child SubGroupSets; the first rows of their sets as parent rows of the child-group queries; the
    child groups' first rows as parent rows of the pod-set queries.  call(jobs, groups, podsets, rows, nodeset_of) -> (ans, sets, masks, res).
    Returns [(queries, rows, (ans, sets, masks, res))] for the three rounds."""
    a = snap.arrays
    kids = {}
    for g, p in enumerate(a["group_parent"].tolist()):
        if p >= 0: kids.setdefault(p, []).append(g)
    jobs = [j for j in range(snap.n_jobs) if int(a["job_root_group"][j]) in kids]
    assert jobs
    rounds = []
    r0 = call(jobs, None, None, None, None)
    rounds.append((np.array([(j, -1, -1, -1) for j in jobs], Q_DT), [], r0))
    rows, q1 = [], []
    for i, j in enumerate(jobs):
        for k in range(r0[0]["first"][i], r0[0]["first"][i] + min(r0[0]["n_sets"][i], max_rows)):
            rows.append(r0[2][k])
            for g in kids[int(a["job_root_group"][j])]: q1.append((j, g, -1, len(rows) - 1))
    q1 = np.array(q1, Q_DT)
    r1 = call(q1["job"], q1["group"], None, rows, q1["nodeset"])
    rounds.append((q1, rows, r1))
    rows2, q2 = [], []
    for i in range(len(q1)):
        for k in range(r1[0]["first"][i], r1[0]["first"][i] + min(r1[0]["n_sets"][i], 2)):
            rows2.append(r1[2][k])
            for s in np.nonzero(a["podset_group"] == q1["group"][i])[0].tolist(): q2.append((int(q1["job"][i]), -1, s, len(rows2) - 1))
    q2 = np.array(q2, Q_DT)
    if len(q2):
        rounds.append((q2, rows2, call(q2["job"], None, q2["podset"], rows2, q2["nodeset"])))
    return rounds


# ---------------------------------------------------------------------------------------------- the host side under the host-only library
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
import test_subset_nodes as ts
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
U32, I64 = C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
lib.kai_subset_nodes.argtypes = [C.c_void_p, C.POINTER(abi.KaiSubsetParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, I64, C.c_void_p, C.POINTER(abi.KaiSubsetResult)]
snap, cfg = ts.replica_scene()
a = snap.arrays
N, W = snap.n_nodes, (snap.n_nodes + 31) // 32
child = int(np.nonzero(a["group_parent"] >= 0)[0][0]); cj = int(a["group_job"][child]); other = int(np.nonzero(a["group_job"] != cj)[0][0])
cps = int(np.nonzero(a["podset_group"] == child)[0][0]); ops = int(np.nonzero(a["podset_job"] != cj)[0][0])
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def call(h, version=1, flags=0, q=((0, -1, -1, -1),), n_rows=0, cap=64, null=(), m=None):
    """-> [status, every output untouched, n_sets_out, result]"""
    qa = np.array(list(q), ts.Q_DT); M = len(qa) if m is None else m
    ans = np.full(max(len(qa), 1) * 6, -7, np.int32); sets = np.full(64 * 4, -8, np.int32); maps = np.full(64 * max(W, 1), 0x99, np.uint32); rows = np.zeros(max(n_rows, 1) * max(W, 1), np.uint32)
    n = C.c_int64(-3); r = abi.KaiSubsetResult(11, 12, 13); pm = abi.KaiSubsetParams(version, flags)
    rc = lib.kai_subset_nodes(h, None if "params" in null else C.byref(pm), None if "queries" in null else qa.ctypes.data, M, None if "rows" in null else rows.ctypes.data, n_rows,
                              None if "answers" in null else ans.ctypes.data, None if "sets" in null else sets.ctypes.data, cap, None if "n" in null else C.byref(n),
                              None if "maps" in null else maps.ctypes.data, None if "result" in null else C.byref(r))
    untouched = bool((ans == -7).all() and (sets == -8).all() and (maps == 0x99).all() and n.value == -3 and (r.n_sets, r.path, r.pad) == (11, 12, 13))
    return [rc, untouched, n.value, [r.n_sets, r.path, r.pad]]
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
res["before_open"] = call(h)
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = image()
bad = {}
bad["version"] = call(h, version=2)
bad["unknown_flags"] = call(h, flags=2)
bad["unknown_flags_high"] = call(h, flags=0x80000001)
bad["null_params"] = call(h, null=("params",))
bad["null_n_sets_out"] = call(h, null=("n",))
bad["null_queries"] = call(h, null=("queries",))
bad["null_answers"] = call(h, null=("answers",))
bad["null_rows_with_count"] = call(h, n_rows=1, null=("rows",))
bad["null_sets_with_capacity"] = call(h, null=("sets",))
bad["negative_queries"] = call(h, m=-1)
bad["negative_rows"] = call(h, n_rows=-1)
bad["negative_capacity"] = call(h, cap=-1)
bad["job_high"] = call(h, q=((snap.n_jobs, -1, -1, -1),))
bad["job_negative"] = call(h, q=((-1, -1, -1, -1),))
bad["group_high"] = call(h, q=((cj, len(a["group_job"]), -1, -1),))
bad["group_below"] = call(h, q=((cj, -2, -1, -1),))
bad["podset_high"] = call(h, q=((cj, -1, snap.n_podsets, -1),))
bad["group_of_another_job"] = call(h, q=((other, child, -1, -1),))
bad["podset_of_another_job"] = call(h, q=((cj, -1, ops, -1),))
bad["group_and_podset"] = call(h, q=((cj, child, cps, -1),))
bad["nodeset_high"] = call(h, q=((0, -1, -1, 1),), n_rows=1)
bad["nodeset_below"] = call(h, q=((0, -1, -1, -2),))
bad["second_query_bad"] = call(h, q=((0, -1, -1, -1), (snap.n_jobs, -1, -1, -1)))
res["image_unchanged"] = image() == img0
res["bad"] = bad
res["empty"] = call(h, q=(), m=0, null=("queries", "answers", "sets", "maps", "rows"), cap=0)
res["image_unchanged_by_empty"] = image() == img0
P = snap.n_pods
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
res["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
# calls that go through (the kernels of the host-only library do nothing: the total that comes back is the zero that was sent)
res["good1"] = call(h, q=((cj, child, -1, -1), (cj, -1, cps, 0), (0, -1, -1, -1)), n_rows=1)[:3]; i1 = image()
res["good2"] = call(h, q=((cj, child, -1, -1), (cj, -1, cps, 0), (0, -1, -1, -1)), n_rows=1)[:3]; i2 = image()
res["engine"] = call(h, flags=1)[:3]; i3 = image()
res["null_optional"] = call(h, null=("maps", "result", "sets"), cap=0)[:3]
d = lambda x, y: dict(allocations=y[1] - x[1], launches=y[3] - x[3], h2d=y[4] - x[4], memsets=y[7] - x[7], pinned=y[8] - x[8])
res["first_call"] = d(img0, i1); res["warm_call"] = d(i1, i2); res["engine_call"] = d(i2, i3)
lib.kai_core_destroy(h)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["sharded"] = call(h2)
lib.kai_core_destroy(h2)
# a snapshot without groups has the root form only
snap3, cfg3, _ = pkg.synth.config(0)
h3 = C.c_void_p(); st3 = snap3.as_struct()
assert lib.kai_core_create(C.byref(cfg3), 1, None, C.byref(h3)) == 0 and lib.kai_session_open(h3, C.byref(st3)) == 0
res["no_groups_root"] = call(h3)[:3]
res["no_groups_podset"] = call(h3, q=((0, -1, 0, -1),))
res["no_groups_group"] = call(h3, q=((0, 0, -1, -1),))
lib.kai_core_destroy(h3)
print(json.dumps(res))
'''


def test_arguments_and_refusals(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["before_open"][:2] == [-6, True], "KAI_ERR_STATE without an open session"
    for k, v in out["bad"].items():
        assert v[:2] == [-1, True], (k, v)
    assert out["image_unchanged"], "a refused call allocated or wrote device memory"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["sharded"][:2] == [-5, True], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["empty"][0] == 0 and out["empty"][2] == 0 and out["empty"][3] == [0, NONE, 0] and out["image_unchanged_by_empty"], "n_queries == 0: KAI_OK without a device call, path NONE"
    for k in ("good1", "good2", "engine", "null_optional", "no_groups_root"):
        assert out[k][0] == 0 and out[k][2] == 0, (k, out[k])
    assert out["no_groups_podset"][:2] == [-1, True] and out["no_groups_group"][:2] == [-1, True], "a snapshot without groups has the root form only"
    # the device side of a call whose total is 0: one upload; the chunk, prep, walk and offsets kernels; the first call of a session allocates the scratch and sends its tables too
    assert out["first_call"]["launches"] == 4 and out["first_call"]["h2d"] == 1 and out["first_call"]["allocations"] == 1 and out["first_call"]["pinned"] > 0
    assert out["warm_call"] == dict(allocations=0, launches=4, h2d=1, memsets=0, pinned=0), out["warm_call"]
    assert out["engine_call"]["launches"] == 4 and out["engine_call"]["h2d"] == 1, out["engine_call"]


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "subset_nodes_sim.cpp")
ACTIONS = {"allocate": 0}


def sim_lib():
    so = os.path.join(ROOT, "tests", "host_sim", "libsubsetnodessim.so")
    deps = glob.glob(os.path.join(ROOT, "tests", "host_sim", "*.?pp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_snsim_run.restype = C.c_int
    lib.kai_snsim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64), C.c_void_p, C.POINTER(abi.KaiSubsetResult), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    return lib


def sim_call(snap, cfg, jobs, groups=None, podsets=None, rows=None, nodeset_of=None, engine=False, lanes=256, wgs=1 << 20, pre=(), post=(), twin=False):
    """kai_subset_nodes on the host simulation behind the actions `pre` -> T.Result(ans, sets, masks, res, unchanged, ops, status, node)"""
    from test_ordered_nodes import words_of
    N, W = snap.n_nodes, max((snap.n_nodes + 31) // 32, 1)
    M = len(jobs)
    per = lambda v: np.full(M, -1, np.int32) if v is None else np.asarray(v, np.int32)
    q = np.zeros(M, Q_DT); q["job"], q["group"], q["podset"], q["nodeset"] = np.asarray(jobs, np.int32), per(groups), per(podsets), per(nodeset_of)
    rows = [] if rows is None else list(rows)
    words = np.ascontiguousarray(words_of(rows, N))
    D = len(snap.arrays["domain_parent"]) if "domain_parent" in snap.arrays else 0
    cap = M * (D + 2)
    ans = np.zeros(max(M, 1), A_DT); sets = np.zeros(max(cap, 1), S_DT); maps = np.zeros((max(cap, 1), W), np.uint32)
    n, res, status, same, n_ops = C.c_int64(0), abi.KaiSubsetResult(), C.c_int(99), C.c_int(0), C.c_int64(0)
    P = snap.n_pods
    ops = np.zeros(8 * P + 64, T.pkg.core._OP_DTYPE); st = np.zeros(max(P, 1), np.int32); nd = np.zeros(max(P, 1), np.int32)
    pre_a = np.array([ACTIONS[x] for x in pre], np.int32); post_a = np.array([ACTIONS[x] for x in post], np.int32)
    s = snap.as_struct()
    rc = sim_lib().kai_snsim_run(C.addressof(cfg), C.addressof(s), pre_a.ctypes.data if len(pre_a) else None, len(pre_a), 0, 1 if twin else 0, abi.SUBSET_ENGINE_PATH if engine else 0, lanes, wgs,
                                 q.ctypes.data, M, words.ctypes.data, len(rows), ans.ctypes.data, sets.ctypes.data, cap, C.byref(n), maps.ctypes.data, C.byref(res), C.byref(status), C.byref(same),
                                 post_a.ctypes.data if len(post_a) else None, len(post_a), ops.ctypes.data, len(ops), C.byref(n_ops), st.ctypes.data, nd.ctypes.data)
    assert rc == 0, rc
    total = int(n.value)
    bits = (maps[:total, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return T.Result(q=q, rows=rows, call_status=status.value, ans=ans[:M], sets=sets[:total].copy(), masks=bits.reshape(total, W * 32)[:, :N].astype(bool), res=res, unchanged=same.value,
                    ops=ops[:n_ops.value].copy(), pod_status=st[:P], pod_node=nd[:P])


def both_paths(snap, cfg, jobs, what, want_path=WIDE, pods=False, state=None, **kw):
    """both paths on the host simulation, against each other, the oracle (root queries over all nodes) and "changes nothing" -> the oracle's answers"""
    w, e = sim_call(snap, cfg, jobs, **kw), sim_call(snap, cfg, jobs, engine=True, **kw)
    for r, name in ((w, "chip-wide allowed"), (e, "engine path")):
        assert r.call_status == 0 and r.unchanged == 1, f"{what} ({name}): status {r.call_status}, unchanged {r.unchanged}"
        check_consistent(snap, r.q, r.rows, r.ans, r.sets, r.masks, r.res, f"{what} ({name})")
    assert w.res.path == want_path and e.res.path == ENGINE, (what, w.res.path, e.res.path)
    assert same_answers((w.ans, w.sets, w.masks), (e.ans, e.sets, e.masks)), f"{what}: the two paths differ"
    return check_against_oracle(state if state is not None else snap, cfg, jobs, w.ans, w.sets, w.masks, what, pods=pods)


@pytest.mark.parametrize("i", range(len(KAT.CASES) + 3 + len(KAT.SCENES)))
def test_sim_the_references_tables(i):
    name, snap, cfg = kat_scenes()[i]
    jobs = [snap.job_names.index("test-job")]
    refs = both_paths(snap, cfg, jobs, name, pods=True)
    want = {"284:topology not found": NO_TOPOLOGY, "320:insufficient allocatable pods - no domains found": NO_FIT, "484:constraint names a level the topology does not have": BAD_LEVEL,
            "no room in the zone": NO_FIT}.get(name, OK)
    assert refs[0][0] == want, (name, refs[0][0])


SHAPES = [(70, 2, 3), (300, 2, 70), (300, 3, 5)]


@pytest.mark.parametrize("N,zones,racks", SHAPES)
def test_sim_synthetic_against_the_oracle(N, zones, racks):
    snap, cfg = synthetic(N, zones, racks)
    jobs = topology_jobs(snap)
    refs = [oracle_answer(snap, cfg, j) for j in jobs]
    lens = [len(s) for _, s in refs]
    assert 0 in lens and max(lens) > 1, "empty and longer lists occur in the oracle's answers"
    if racks == 70: assert 1 in lens and max(lens) >= 40, "a single set and a list of 40 sets or more occur"
    assert {NO_TOPOLOGY, BAD_LEVEL, OK} <= {s for s, _ in refs}
    unl = snap.arrays["node_domain"][0] < 0
    assert unl.sum() >= N // 20 and not any(unl[list(s)].any() for _, ss in refs for s in ss if len(s) < N), "no set of a domain holds an unlabelled node"
    both_paths(snap, cfg, jobs, f"N {N}")
    if N == 70:  # other workgroup shapes and a grid below the queries: the same answers
        ref = sim_call(snap, cfg, jobs)
        for lanes, wgs in ((100, 3), (64, 1), (1, 1 << 20)):
            r = sim_call(snap, cfg, jobs, lanes=lanes, wgs=wgs)
            assert same_answers((r.ans, r.sets, r.masks), (ref.ans, ref.sets, ref.masks)), (lanes, wgs)


def test_sim_a_state_only_an_action_reaches():
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    twin = sim_call(snap, cfg, jobs, pre=("allocate",), twin=True)
    after = state_snapshot(snap, twin.pod_status, twin.pod_node)
    refs = both_paths(snap, cfg, jobs, "after allocate", state=after, pre=("allocate",))
    fresh = [oracle_answer(snap, cfg, j) for j in jobs]
    assert sum(x != y for x, y in zip(refs, fresh)) * 3 >= len(jobs), "at least a third of the answers differ from the fresh session's: the test cannot pass on stale state"


def test_sim_sub_groups_and_parent_rows():
    snap, cfg = replica_scene()
    a = snap.arrays
    roots = both_paths(snap, cfg, np.arange(snap.n_jobs, dtype=np.int32), "replica roots")
    assert any(s == OK for s, _ in roots)
    call_w = lambda jobs, groups, podsets, rows, ns: (lambda r: (r.ans, r.sets, r.masks, r))(sim_call(snap, cfg, jobs, groups, podsets, rows, ns))
    call_e = lambda jobs, groups, podsets, rows, ns: (lambda r: (r.ans, r.sets, r.masks, r))(sim_call(snap, cfg, jobs, groups, podsets, rows, ns, engine=True))
    rw, re = inner_walk(call_w, snap), inner_walk(call_e, snap)
    assert len(rw) == len(re) == 3
    proper, empty = False, False
    for (q, rows, w), (_q, _rows, e) in zip(rw, re):
        assert w[3].call_status == 0 and e[3].call_status == 0 and w[3].unchanged and e[3].unchanged
        assert w[3].res.path == WIDE and e[3].res.path == ENGINE
        check_consistent(snap, q, rows, w[0], w[1], w[2], w[3].res, "inner")
        assert same_answers(w, e), "the chip-wide path against the engine path on the inner queries"
        proper |= any(0 < r.sum() < snap.n_nodes for r in rows)
        empty |= bool(len(rows) and (w[0]["n_sets"] == 0).any())
    assert proper, "an inner query has a parent row that is a proper subset of the nodes"
    assert empty, "an inner query has no set"


def test_sim_the_next_allocate_is_the_twins():
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    twin = sim_call(snap, cfg, jobs, post=("allocate",), twin=True)
    for engine in (False, True):
        r = sim_call(snap, cfg, jobs, engine=engine, post=("allocate",))
        assert r.unchanged == 1 and r.ops.tobytes() == twin.ops.tobytes() and len(r.ops) > 0 and np.array_equal(r.pod_status, twin.pod_status) and np.array_equal(r.pod_node, twin.pod_node)


def test_sim_sessions_the_chip_wide_path_does_not_take():
    """fraction pods (shared GPUs) send the call to the engine path; its answers are still the oracle's"""
    snap, cfg = synthetic(70, 2, 3)
    synth.add_fractions(snap, 7, frac=0.3)
    both_paths(snap, cfg, topology_jobs(snap), "fractions", want_path=ENGINE)


REVERSED = r'''
import json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import test_subset_nodes as ts
snap, cfg = ts.synthetic(70, 2, 3)
r = ts.sim_call(snap, cfg, ts.topology_jobs(snap))
print(json.dumps([r.ans.tobytes().hex(), r.sets.tobytes().hex(), r.masks.tobytes().hex()]))
'''


@pytest.mark.parametrize("order", ["1", "2"])
def test_kernel_bodies_with_other_wave_orders(order):
    """the emulator's waves take their turns in reverse / at random (KW_EMU_ORDER, read once per process: a fresh one): sums that leaned on the waves' order would differ"""
    snap, cfg = synthetic(70, 2, 3)
    ref = sim_call(snap, cfg, topology_jobs(snap))
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + REVERSED], env=dict(os.environ, KW_EMU_ORDER=order), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == [ref.ans.tobytes().hex(), ref.sets.tobytes().hex(), ref.masks.tobytes().hex()]


def test_stand_alone_program(tmp_path):
    """the fixed case behind -DKAI_SNSIM_MAIN builds and passes: 256 / 100 / 1 lanes, small and large grids, both paths, fresh and behind an allocate, the twin, the
    capacity protocol (the count needed, nothing written)"""
    exe = str(tmp_path / "subset_nodes_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKAI_SNSIM_MAIN", "-o", exe, SIM_SRC])
    for order in ("0", "1"):
        r = subprocess.run([exe], env=dict(os.environ, KW_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "subset_nodes_sim: ok" in r.stdout, (order, r.stdout[-2000:], r.stderr[-2000:])


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan (a program of its own: nothing is loaded into python)"""
    exe = str(tmp_path / "subset_nodes_sim_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKAI_SNSIM_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0"), capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "subset_nodes_sim: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
