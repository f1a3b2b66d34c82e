"""kai_subset_nodes on the MI355X.  The expected node sets come from the oracle's subSetNodesFn (kai_oracle_subset_nodes_all, kai_oracle_subset_nodes for the status,
kai_oracle_tree_allocatable for AllocatablePods), called per job on the snapshot that equals the session's state — for a state after an action the original with the handle's
kai_pod_states read-back written into pod_status / pod_node — never from the code under test; "changes nothing" from the handle's own read-backs and from a twin handle that never
made the call.  Both paths are asked everywhere and must agree record for record, bitmap word for word.  The same scenes run with emulated lanes in tests/test_subset_nodes.py."""
import ctypes as C

import numpy as np
import pytest

import kai_testlib as T
import test_oracle_topology_kat as KAT
from test_gpu_parity import gpu  # noqa: F401  (fixture)
from test_gpu_session_update import assert_readback_equal, readback
from test_subset_nodes import (A_DT, BAD_LEVEL, ENGINE, NO_FIT, NO_TOPOLOGY, NONE, OK, Q_DT, S_DT, SHAPES, WIDE, check_against_oracle, check_consistent, inner_walk, kat_scenes,
                               oracle_answer, replica_scene, same_answers, state_snapshot, synthetic, topology_jobs)

pytestmark = pytest.mark.gpu
abi = T.abi
synth = T.pkg.synth


def rows_of(arr):
    return [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["stmt"])) for o in arr]


def both(ssn, snap, jobs, what, groups=None, podsets=None, rows=None, nodeset_of=None, want_path=WIDE):
    """both paths at the session's current state: consistent, equal, the paths as expected -> the chip-wide call's (ans, sets, masks, res)"""
    w = ssn.subset_nodes(jobs, groups, podsets, rows, nodeset_of)
    e = ssn.subset_nodes(jobs, groups, podsets, rows, nodeset_of, engine_path=True)
    M = len(w[0])
    q = np.zeros(M, Q_DT); q["job"] = np.asarray(jobs, np.int32)
    q["nodeset"] = -1 if nodeset_of is None else np.asarray(nodeset_of, np.int32)
    for r, name in ((w, "chip-wide allowed"), (e, "engine path")):
        check_consistent(snap, q, [] if rows is None else rows, r[0], r[1], r[2], r[3], f"{what} ({name})")
    assert w[3].path == want_path and e[3].path == ENGINE, (what, w[3].path, e[3].path)
    assert same_answers(w, e), f"{what}: the two paths differ"
    return w


def against_oracle(ssn, snap, cfg, jobs, what, want_path=WIDE, pods=False, state=None):
    """root queries over all nodes, both paths, against the oracle on the snapshot that equals the session's state -> (the oracle's answers, the call's)"""
    if state is None:
        st, nd = ssn.pod_states()
        state = state_snapshot(snap, st, nd)
    w = both(ssn, snap, jobs, what, want_path=want_path)
    return check_against_oracle(state, cfg, jobs, w[0], w[1], w[2], what, pods=pods), w


N_KAT = len(KAT.CASES) + 3 + len(KAT.SCENES)


def test_gpu_the_references_tables(gpu):
    """every scene of tests/test_oracle_topology_kat.py: status, n_sets, every set, AllocatablePods"""
    seen = set()
    scenes = kat_scenes()
    assert len(scenes) == N_KAT
    for name, snap, cfg in scenes:
        with T.pkg.KaiCore(cfg) as core:
            ssn = core.open_session(snap)
            refs, _ = against_oracle(ssn, snap, cfg, [snap.job_names.index("test-job")], name, pods=True, state=snap)
            seen.add(refs[0][0])
            ssn.close()
    assert seen == {OK, NO_TOPOLOGY, NO_FIT, BAD_LEVEL}


@pytest.mark.parametrize("N,zones,racks", SHAPES)
def test_gpu_synthetic_fresh_against_the_oracle(gpu, N, zones, racks):
    snap, cfg = synthetic(N, zones, racks)
    jobs = topology_jobs(snap)
    refs = [oracle_answer(snap, cfg, j) for j in jobs]
    lens = [len(s) for _, s in refs]
    assert 0 in lens and max(lens) > 1, "empty and longer lists occur in the oracle's answers"
    if racks == 70: assert 1 in lens and max(lens) >= 40, "a single set and a list of 40 sets or more occur"
    assert {NO_TOPOLOGY, BAD_LEVEL, OK} <= {s for s, _ in refs}
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got, w = against_oracle(ssn, snap, cfg, jobs, f"N {N}", state=snap)
        assert got == refs
        unl = snap.arrays["node_domain"][0] < 0
        assert unl.sum() >= N // 20 and not w[2][w[1]["domain"] != abi.SUBSET_PARENT][:, unl].any(), "no set of a domain holds an unlabelled node"
        ssn.close()


def test_gpu_a_state_only_an_action_reaches(gpu):
    """the N = 300 scene after one allocate, then after a kai_session_update that makes a rack's nodes NotReady and changes one node's allocatable"""
    snap, cfg = synthetic(300, 2, 70)
    jobs = topology_jobs(snap)
    fresh = [oracle_answer(snap, cfg, j) for j in jobs]
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        assert len(ssn.execute("allocate")) > 0
        refs, _ = against_oracle(ssn, snap, cfg, jobs, "after allocate")
        assert sum(x != y for x, y in zip(refs, fresh)) * 3 >= len(jobs), "at least a third of the answers differ from the fresh session's: the test cannot pass on stale state"
        ssn.close()
        ssn = core.open_session(snap)
        a = snap.arrays
        rack = int(a["node_domain"][1][a["node_domain"][1] >= 0][7])
        nodes = np.nonzero(a["node_domain"][1] == rack)[0]
        other = int(np.nonzero((a["node_domain"][1] >= 0) & (a["node_domain"][1] != rack))[0][3])
        flags = a["node_flags"][nodes] | abi.NODE_NOT_READY
        ssn.update([], [], [], nodes=nodes, node_flags=flags)
        alloc = a["node_allocatable"][:, [other]].copy(); alloc[abi.RES_GPU, 0] += 4; alloc[abi.RES_CPU, 0] += 8000
        ssn.update([], [], [], nodes=[other], node_allocatable=alloc)
        after, _ = against_oracle(ssn, ssn.snap, cfg, jobs, "after the update", state=ssn.snap)
        assert after != fresh, "the update shows in the oracle's answers"
        ssn.close()


def test_gpu_sub_groups_and_parent_rows(gpu):
    snap, cfg = replica_scene()
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        roots, _ = against_oracle(ssn, snap, cfg, np.arange(snap.n_jobs, dtype=np.int32), "replica roots", state=snap)
        assert any(s == OK for s, _ in roots)
        call = lambda engine: (lambda jobs, groups, podsets, rows, ns: ssn.subset_nodes(jobs, groups, podsets, rows, ns, engine_path=engine))
        rw, re = inner_walk(call(False), snap), inner_walk(call(True), snap)
        assert len(rw) == len(re) == 3
        proper = empty = False
        for (q, rows, w), (_q, _rows, e) in zip(rw, re):
            assert w[3].path == WIDE and e[3].path == ENGINE
            check_consistent(snap, q, rows, w[0], w[1], w[2], w[3], "inner")
            assert same_answers(w, e), "the chip-wide path against the engine path on the inner queries"
            proper |= any(0 < r.sum() < snap.n_nodes for r in rows)
            empty |= bool(len(rows) and (w[0]["n_sets"] == 0).any())
        assert proper, "an inner query has a parent row that is a proper subset of the nodes"
        assert empty, "an inner query has no set"
        ssn.close()


def test_gpu_many_and_repeated_queries(gpu):
    """M = 1 100 queries cycling over the distinct ones: more than the capped grid, so the grid-stride loops run"""
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    M = 1100
    many = np.resize(jobs, M)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        base = both(ssn, snap, jobs, "the distinct queries")
        big = both(ssn, snap, many, "1 100 queries")
        assert np.array_equal(big[0]["first"], np.concatenate([[0], np.cumsum(big[0]["n_sets"])[:-1]])), "first is the running sum of n_sets"
        for i in range(M):
            b = i % len(jobs)
            for f in ("status", "n_sets", "tasks", "common_domain"): assert big[0][f][i] == base[0][f][b], (i, f)
            sl_b, sl_i = slice(base[0]["first"][b], base[0]["first"][b] + base[0]["n_sets"][b]), slice(big[0]["first"][i], big[0]["first"][i] + big[0]["n_sets"][i])
            assert big[1][sl_i].tobytes() == base[1][sl_b].tobytes() and np.array_equal(big[2][sl_i], base[2][sl_b]), f"query {i}: equal queries get equal answers"
        ssn.close()


def test_gpu_composition_with_best_nodes(gpu):
    """rows of bitmaps_out as node sets of kai_best_nodes: every answered node lies in its set, and every answer equals kai_best_node with the set given as an index list"""
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    a = snap.arrays
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        ans, sets, masks, _res = ssn.subset_nodes(jobs)
        pods, rows, row_of = [], [], []
        for i, j in enumerate(jobs):
            pending = [p for p in range(a["job_first_pod"][j], a["job_first_pod"][j] + a["job_n_pods"][j]) if a["pod_status"][p] == abi.POD_STATUS["Pending"]]
            for k in range(ans["first"][i], ans["first"][i] + min(ans["n_sets"][i], 3)):
                if not pending: continue
                rows.append(masks[k]); pods.append(pending[0]); row_of.append(len(rows) - 1)
        assert len(rows) >= 10
        node, pipe = ssn.best_nodes(pods, rows, row_of)
        assert (node >= 0).any()
        for t in range(len(pods)):
            if node[t] >= 0: assert rows[row_of[t]][node[t]], "an answered node lies outside its set"
            one = ssn.best_node(pods[t], nodeset=np.nonzero(rows[row_of[t]])[0].tolist())
            assert (int(node[t]), bool(pipe[t])) == (int(one[0]), bool(one[1])) or (node[t] < 0 and one[0] < 0), (t, node[t], one)
        ssn.close()


@pytest.mark.parametrize("scene", ["synthetic", "replica"])
@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_the_call_changes_nothing(gpu, scene, engine):
    snap, cfg = synthetic(300, 2, 70) if scene == "synthetic" else replica_scene()
    jobs = topology_jobs(snap) if scene == "synthetic" else np.arange(snap.n_jobs, dtype=np.int32)
    with T.pkg.KaiCore(cfg) as ca, T.pkg.KaiCore(cfg) as cb:
        sa, sb = ca.open_session(snap), cb.open_session(snap)
        before, stats0 = readback(sa), bytes(sa.stats())
        first = sa.subset_nodes(jobs, engine_path=engine)
        if scene == "replica": inner_walk(lambda j, g, p, r, n: sa.subset_nodes(j, g, p, r, n, engine_path=engine), snap)
        assert_readback_equal(readback(sa), before)
        assert_readback_equal(readback(sa), readback(sb))
        assert bytes(sa.stats()) == stats0, "kai_action_stats_get"  # (the twin's statistics hold its own open's times)
        pending = np.nonzero(sa.pod_states()[0] == abi.POD_STATUS["Pending"])[0][:32]
        na, pa = sa.best_nodes(pending); nb, pb = sb.best_nodes(pending)
        assert np.array_equal(na, nb) and np.array_equal(pa, pb), "best nodes"
        oa, ob = sa.execute("allocate"), sb.execute("allocate")
        assert rows_of(oa) == rows_of(ob) and len(oa) > 0, "the allocate behind the call against the twin's"
        assert_readback_equal(readback(sa), readback(sb))
        again = sa.subset_nodes(jobs, engine_path=engine)
        assert not same_answers(first, again) or scene == "replica", "the allocate shows in the answers"
        sa.close(); sb.close()


def test_gpu_sessions_the_chip_wide_path_does_not_take(gpu):
    """fraction pods, and quantities that do not add exactly: the engine path, whose answers are still the oracle's"""
    snap, cfg = synthetic(70, 2, 3)
    synth.add_fractions(snap, 7, frac=0.3)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        against_oracle(ssn, snap, cfg, topology_jobs(snap), "fractions", want_path=ENGINE, state=snap)
        ssn.close()
    snap, cfg = synthetic(70, 2, 3)
    snap.arrays["node_allocatable"][abi.RES_MEM, 3] += 0.5  # (no integer: the sums are not exact in any order)
    snap.finalize()
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        refs, _ = against_oracle(ssn, snap, cfg, topology_jobs(snap), "no exact sums", want_path=ENGINE, state=snap)
        assert any(s == OK for s, _ in refs)
        ssn.close()


def test_gpu_refusals_and_capacity(gpu):
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    M, W = len(jobs), (snap.n_nodes + 31) // 32

    def raw(core, cap, version=1, flags=0, q=None, n_queries=None):
        qa = np.zeros(M, Q_DT); qa["job"] = jobs; qa["group"] = -1; qa["podset"] = -1; qa["nodeset"] = -1
        if q is not None: qa[0] = q
        ans = np.full(M * 6, -7, np.int32); sets = np.full(max(cap, 1) * 4, -8, np.int32); maps = np.full(max(cap, 1) * W, 0x99, np.uint32); n = C.c_int64(-3); r = abi.KaiSubsetResult(11, 12, 13)
        pm = abi.KaiSubsetParams(version, flags)
        rc = core.lib.kai_subset_nodes(core.handle, C.byref(pm), qa.ctypes.data_as(C.POINTER(abi.KaiSubsetQuery)), M if n_queries is None else n_queries, None, 0,
                                       ans.ctypes.data_as(C.POINTER(abi.KaiSubsetAnswer)), sets.ctypes.data_as(C.POINTER(abi.KaiNodeSet)), cap, C.byref(n),
                                       maps.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(r))
        untouched = bool((ans == -7).all() and (sets == -8).all() and (maps == 0x99).all() and (r.n_sets, r.path, r.pad) == (11, 12, 13))
        return rc, n.value, untouched

    with T.pkg.KaiCore(cfg) as core:
        assert raw(core, 64) == (-6, -3, True), "KAI_ERR_STATE without an open session"
        ssn = core.open_session(snap)
        before = readback(ssn)
        assert raw(core, 64, version=2) == (-1, -3, True) and raw(core, 64, flags=4) == (-1, -3, True) and raw(core, -1) == (-1, -3, True)
        assert raw(core, 64, q=(snap.n_jobs, -1, -1, -1)) == (-1, -3, True) and raw(core, 64, q=(0, -1, -1, 0)) == (-1, -3, True) and raw(core, 64, q=(0, 0, 0, -1)) == (-1, -3, True)
        total = len(ssn.subset_nodes(jobs)[1])
        assert total > 1
        for flags in (0, abi.SUBSET_ENGINE_PATH):
            assert raw(core, total - 1, flags=flags) == (-4, total, True), "KAI_ERR_CAPACITY: *n_sets_out holds the number needed, the other outputs are untouched"
            assert raw(core, total, flags=flags)[:2] == (0, total)
        rc, n, untouched = raw(core, 0, n_queries=0)
        assert (rc, n) == (0, 0), "n_queries == 0: KAI_OK"
        assert_readback_equal(readback(ssn), before)
        ssn.close()
        assert raw(core, 64) == (-6, -3, True), "KAI_ERR_STATE after kai_session_close"
    with T.pkg.KaiCore(cfg, world=2, rank=0, allgather=lambda send, recv, nbytes: 1) as grp:
        assert raw(grp, 64) == (-5, -3, True), "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
