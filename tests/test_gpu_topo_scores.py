"""kai_subset_nodes_scored and kai_ordered_nodes_scored on the MI355X.  The expected scores come from the oracle's calculateNodeScores (kai_oracle_topology_scores), called per
job on the snapshot that equals the session's state; the order a gang is placed in from the oracle's allocate action; "changes nothing" from the handle's own read-backs and
from a twin handle that never made the call.  Both paths are asked everywhere and must agree byte for byte, and everything kai_subset_nodes returns must come back unchanged.
The same scenes run with emulated lanes in tests/test_topo_scores.py, whose helpers are used here."""
import ctypes as C

import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import gpu  # noqa: F401  (fixture)
from test_gpu_session_update import assert_readback_equal, readback
from test_subset_nodes import BAD_LEVEL, ENGINE, NO_FIT, OK, Q_DT, SHAPES, WIDE, check_consistent, inner_walk, kat_scenes, replica_scene, same_answers, state_snapshot, synthetic, topology_jobs
from test_topo_scores import (EMPTY_ROW, NO_SCORE, NONE_ROW, R_DT, SQ_DT, check_rows, check_scored_lists, gang_scene, list_queries, node_scores, oracle_scores, score_scene, scored_case,
                              three_level_scene, walk_the_gang)
from test_ordered_nodes import as_lists

pytestmark = pytest.mark.gpu
abi = T.abi
synth = T.pkg.synth


def rows_of(arr):
    return [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["stmt"])) for o in arr]


def scored_both(ssn, snap, cfg, jobs, what, groups=None, podsets=None, rows=None, nodeset_of=None, want_path=WIDE, state=None, oracle=True):
    """the scored call on both paths at the session's current state: consistent, equal byte for byte, kai_subset_nodes' outputs unchanged, and (root queries over all nodes)
    the oracle's scores on the snapshot that equals the state -> (T.Result of the chip-wide call, the oracle's per-node scores or None per job)"""
    plain = ssn.subset_nodes(jobs, groups, podsets, rows, nodeset_of)
    w = ssn.subset_nodes_scored(jobs, groups, podsets, rows, nodeset_of)
    e = ssn.subset_nodes_scored(jobs, groups, podsets, rows, nodeset_of, engine_path=True)
    M = len(w[0])
    q = np.zeros(M, Q_DT); q["job"] = np.asarray(jobs, np.int32)
    q["nodeset"] = -1 if nodeset_of is None else np.asarray(nodeset_of, np.int32)
    out = []
    for r, name in ((w, "chip-wide allowed"), (e, "engine path")):
        res = T.Result(q=q, ans=r[0], sets=r[1], masks=r[2], score_rows=r[3], deciles=r[4], res=r[5])
        check_consistent(snap, q, [] if rows is None else rows, r[0], r[1], r[2], r[5], f"{what} ({name})")
        check_rows(snap, res, f"{what} ({name})")
        out.append(res)
    assert w[5].path == want_path and e[5].path == ENGINE, (what, w[5].path, e[5].path)
    assert same_answers(w, plain) and w[5].path == plain[3].path and w[5].n_sets == plain[3].n_sets, f"{what}: kai_subset_nodes' outputs differ"
    assert same_answers(w, e), f"{what}: the two paths' sets differ"
    assert w[3].tobytes() == e[3].tobytes() and w[4].tobytes() == e[4].tobytes(), f"{what}: the two paths' scores differ"
    refs = []
    if oracle:
        if state is None:
            st, nd = ssn.pod_states()
            state = state_snapshot(snap, st, nd)
        for i, j in enumerate(jobs):
            ref = oracle_scores(state, cfg, j)
            refs.append(ref)
            if ref is None:
                assert w[0]["status"][i] in (BAD_LEVEL, abi.SUBSET_NO_TOPOLOGY), f"{what} job {j}: the oracle's function returned an error, the call says {w[0]['status'][i]}"
                continue
            got = node_scores(snap, w[3][i], w[4][i])
            assert np.array_equal(got, ref), f"{what} job {j}: scores differ from the oracle's at nodes {np.nonzero(got != ref)[0][:8].tolist()}"
    return out[0], refs


def test_gpu_scores_on_the_references_tables(gpu):
    """every scene of tests/test_oracle_topology_kat.py and the three of TestCalculateNodeScores (deciles 10; 3 / 6 / 10; 2 / 5 / 7 / 10)"""
    kinds = set()
    for name, snap, cfg in kat_scenes():
        with T.pkg.KaiCore(cfg) as core:
            ssn = core.open_session(snap)
            w, _ = scored_both(ssn, snap, cfg, [snap.job_names.index("test-job")], name, state=snap)
            kinds.add(int(min(w.score_rows["level_row"][0], 0)))
            ssn.close()
    assert kinds == {0, NONE_ROW}
    for racks, want in (({"rack1": [1, 1]}, {"rack1-n0": 10, "rack1-n1": 10}), ({"rack3": [1], "rack2": [2], "rack1": [3]}, {"rack1-n0": 10, "rack2-n0": 6, "rack3-n0": 3}),
                        ({"rack4": [1], "rack3": [2], "rack2": [3], "rack1": [4]}, {"rack1-n0": 10, "rack2-n0": 7, "rack3-n0": 5, "rack4-n0": 2})):
        snap, cfg = score_scene(racks)
        with T.pkg.KaiCore(cfg) as core:
            ssn = core.open_session(snap)
            w, refs = scored_both(ssn, snap, cfg, [0], str(racks), state=snap)
            got = node_scores(snap, w.score_rows[0], w.deciles[0])
            assert {snap.node_names[n]: got[n] for n in range(snap.n_nodes)} == {k: v * abi.TOPO_SCORE_UNIT for k, v in want.items()} and refs[0] is not None
            ssn.close()


@pytest.mark.parametrize("N,zones,racks", SHAPES)
def test_gpu_scores_synthetic_against_the_oracle(gpu, N, zones, racks):
    snap, cfg = synthetic(N, zones, racks)
    jobs = topology_jobs(snap)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        w, refs = scored_both(ssn, snap, cfg, jobs, f"N {N}", state=snap)
        scored = [r for r in refs if r is not None and (r >= 0).any()]
        assert len(scored) == (3 if N == 70 else 5) and all((r < 0).any() for r in scored), "gangs with scores, unscored (unlabelled) nodes in every row"
        if N == 300: assert all({int(v // abi.TOPO_SCORE_UNIT) for v in r[r >= 0]} == set(range(11)) for r in scored), "every decile 0 .. 10"
        assert NONE_ROW in set(w.score_rows["level_row"].tolist())
        ssn.close()


def test_gpu_three_levels(gpu):
    snap, cfg = three_level_scene()
    a = snap.arrays
    jobs = [snap.job_names.index(x) for x in ("zone-block", "zone-rack", "none-rack", "block-rack", "too-large")]
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        w, refs = scored_both(ssn, snap, cfg, jobs, "three levels", state=snap)
        assert [int(x) for x in w.score_rows["level_row"]] == [1, 2, 2, 2, NONE_ROW] and [int(x) for x in w.score_rows["n_scored"][:4]] == [6, 24, 24, 24]
        assert all(r is not None for r in refs) and len(set(refs[1][refs[1] >= 0].tolist())) == 11
        zone0, block1 = a["node_domain"][0] == a["node_domain"][0][0], a["node_domain"][1] == a["node_domain"][1][16]
        r, _ = scored_both(ssn, snap, cfg, [jobs[0], jobs[1], jobs[0], jobs[1]], "three levels, parent rows", rows=[zone0, block1], nodeset_of=[0, 0, 1, 1], oracle=False)
        assert [tuple(x) for x in r.score_rows] == [(1, 3), (2, 12), (1, 1), (2, 4)]
        assert r.deciles[2][r.deciles[2] != NO_SCORE].tolist() == [10] and np.nonzero(r.deciles[2] != NO_SCORE)[0][0] == a["node_domain"][1][16]
        ssn.close()


@pytest.mark.parametrize("seed", [7, 6])
def test_gpu_sub_groups_and_parent_rows(gpu, seed):
    snap, cfg = replica_scene(seed)
    a = snap.arrays
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        roots, _ = scored_both(ssn, snap, cfg, np.arange(snap.n_jobs, dtype=np.int32), "replica roots", state=snap)
        assert (roots.score_rows["level_row"] == NONE_ROW).any() and (roots.score_rows["level_row"] >= 0).sum() == (3 if seed == 6 else 0)
        keep = {}
        def call(engine):
            def f(jobs, groups, podsets, rows, ns):
                r = ssn.subset_nodes_scored(jobs, groups, podsets, rows, ns, engine_path=engine)
                keep.setdefault(engine, []).append(r)
                return r[0], r[1], r[2], r[5]
            return f
        rw, re = inner_walk(call(False), snap), inner_walk(call(True), snap)
        assert len(rw) == len(re) == 3
        for k, ((q, rows, w), (_q, _rows, e)) in enumerate(zip(rw, re)):
            fw, fe = keep[False][k], keep[True][k]
            assert w[3].path == WIDE and e[3].path == ENGINE and same_answers(w, e) and fw[3].tobytes() == fe[3].tobytes() and fw[4].tobytes() == fe[4].tobytes(), "the two paths on the inner queries"
            check_rows(snap, T.Result(q=q, score_rows=fw[3], deciles=fw[4]), "inner")
            for i in range(len(q)):
                g, s = int(q["group"][i]), int(q["podset"][i])
                grp = int(a["job_root_group"][q["job"][i]]) if g < 0 and s < 0 else g
                topo, pref = (a["podset_topology"][s], a["podset_preferred_level"][s]) if s >= 0 else (a["group_topology"][grp], a["group_preferred_level"][grp])
                has = fw[3]["level_row"][i] != NONE_ROW
                if topo < 0 or pref < 0 or w[0]["tasks"][i] == 0: assert not has, (q[i], w[0][i], fw[3][i])
                elif w[0]["status"][i] in (OK, BAD_LEVEL): assert has, (q[i], w[0][i], fw[3][i])
        ssn.close()


@pytest.mark.parametrize("N,zones,racks", [(70, 2, 3), (300, 3, 5)])
def test_gpu_scored_lists(gpu, N, zones, racks):
    """k = 1, 8, 64 with a Releasing pod in the scene (is_pipeline): N = 70 has three bitmap words and a partial last stride, N = 300 more nodes than a workgroup's stride"""
    snap, cfg = scored_case(N, zones, racks, releasing=True)
    assert (snap.arrays["pod_status"] == abi.POD_STATUS["Releasing"]).any()
    jobs = topology_jobs(snap)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        sc = ssn.subset_nodes_scored(jobs)
        r = T.Result(ans=sc[0], sets=sc[1], masks=sc[2], score_rows=sc[3], deciles=sc[4])
        pods, ns, rows, so = list_queries(snap, r, jobs)
        assert len(pods) >= 8
        lists = lambda out: as_lists(out[0], out[1], out[2])
        full = lists(ssn.ordered_nodes(pods, 64, rows, ns))
        assert any(0 < len(l) < 64 for l in full) and any(p for l in full for _, p in l), "a complete unscored list and a pipelined entry occur"
        none_rows = np.zeros(len(r.score_rows), R_DT); none_rows["level_row"] = NONE_ROW
        empty_rows = np.zeros(len(r.score_rows), R_DT); empty_rows["level_row"] = EMPTY_ROW
        changed = False
        for k in (1, 8, 64):
            ref = [l[:k] for l in full]
            got = lists(ssn.ordered_nodes_scored(pods, k, rows, ns, r.score_rows, r.deciles, so))
            check_scored_lists(snap, r, pods, ns, rows, so, got, full, k, f"k {k}")
            changed |= any(g and u and g[0] != u[0] for g, u in zip(got, ref))
            assert lists(ssn.ordered_nodes_scored(pods, k, rows, ns, none_rows, r.deciles, so)) == ref, "rows of NONE reproduce kai_ordered_nodes' lists"
            assert lists(ssn.ordered_nodes_scored(pods, k, rows, ns, r.score_rows, r.deciles, None)) == ref, "scores = -1 reproduces kai_ordered_nodes' lists"
            assert lists(ssn.ordered_nodes_scored(pods, k, rows, ns)) == ref, "no rows at all"
            assert all(l == [] for l in lists(ssn.ordered_nodes_scored(pods, k, rows, ns, empty_rows, r.deciles, so))), "an EMPTY row gives n_out = 0"
        assert changed, "the scores change the head of some list"
        ssn.close()


def test_gpu_a_gang_placed_by_queries_lands_where_the_allocate_action_puts_it(gpu):
    snap, cfg = gang_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    lists = lambda out: as_lists(out[0], out[1], out[2])
    with T.pkg.KaiCore(cfg) as core, T.pkg.KaiCore(cfg) as other:
        ssn, twin = core.open_session(snap), other.open_session(snap)
        def subset(jobs):
            w, e = ssn.subset_nodes_scored(jobs), ssn.subset_nodes_scored(jobs, engine_path=True)
            assert w[5].path == WIDE and e[5].path == ENGINE and w[3].tobytes() == e[3].tobytes() and w[4].tobytes() == e[4].tobytes()
            return w[0], w[2], w[3], w[4]
        first_unscored, mine = walk_the_gang(snap, cfg, ref, subset, lambda *a: lists(ssn.ordered_nodes_scored(*a)), lambda *a: lists(ssn.ordered_nodes(*a[:4])), ssn.apply_ops)
        assert first_unscored != mine[0][2], "the unscored kai_ordered_nodes puts the first pod elsewhere: the gap the scored call closes"
        assert len(twin.execute("allocate")) == len(ref.ops)
        assert_readback_equal(readback(ssn), readback(twin))
        st, nd = ssn.pod_states()
        assert np.array_equal(st, ref.pod_status) and np.array_equal(nd, ref.pod_node)
        ssn.close(); twin.close()


def test_gpu_many_and_repeated_queries(gpu):
    """M = 1 100 queries cycling over the distinct ones: more than the capped grid of both kernels, so the grid-stride loops run and the per-workgroup tables are reused"""
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    M = 1100
    many = np.resize(jobs, M)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        base, _ = scored_both(ssn, snap, cfg, jobs, "the distinct queries", oracle=False)
        big, _ = scored_both(ssn, snap, cfg, many, "1 100 queries", oracle=False)
        idx = np.arange(M) % len(jobs)
        assert big.score_rows.tobytes() == base.score_rows[idx].tobytes() and big.deciles.tobytes() == base.deciles[idx].tobytes(), "equal queries get equal rows"
        pods, ns, rows, so = list_queries(snap, base, jobs)
        rep = np.arange(M) % len(pods)
        lists = lambda out: as_lists(out[0], out[1], out[2])
        few = lists(ssn.ordered_nodes_scored(pods, 8, rows, ns, base.score_rows, base.deciles, so))
        lots = lists(ssn.ordered_nodes_scored(np.asarray(pods)[rep], 8, rows, np.asarray(ns)[rep], big.score_rows, big.deciles, np.asarray(so)[rep] + len(jobs) * (np.arange(M) % 7)))
        # (query x names row so[x] + a multiple of len(jobs): another copy of the same row)
        assert lots == [few[x] for x in rep], "equal queries get equal lists"
        ssn.close()


def test_gpu_a_state_only_an_action_reaches(gpu):
    """the N = 300 scene after one allocate, then after a kai_session_update that makes a rack's nodes NotReady and changes one node's allocatable"""
    snap, cfg = synthetic(300, 2, 70)
    jobs = topology_jobs(snap)
    fresh = [oracle_scores(snap, cfg, j) for j in jobs]
    differs = lambda refs: sum(not (x is None and y is None) and (x is None or y is None or not np.array_equal(x, y)) for x, y in zip(refs, fresh))
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        assert len(ssn.execute("allocate")) > 0
        _, refs = scored_both(ssn, snap, cfg, jobs, "after allocate")
        assert differs(refs) >= 1, "the allocate shows in the oracle's scores: the test cannot pass on stale state"
        ssn.close()
        ssn = core.open_session(snap)
        a = snap.arrays
        rack = int(a["node_domain"][1][a["node_domain"][1] >= 0][7])
        nodes = np.nonzero(a["node_domain"][1] == rack)[0]
        other = int(np.nonzero((a["node_domain"][1] >= 0) & (a["node_domain"][1] != rack))[0][3])
        ssn.update([], [], [], nodes=nodes, node_flags=a["node_flags"][nodes] | abi.NODE_NOT_READY)
        alloc = a["node_allocatable"][:, [other]].copy(); alloc[abi.RES_GPU, 0] += 4; alloc[abi.RES_CPU, 0] += 8000
        ssn.update([], [], [], nodes=[other], node_allocatable=alloc)
        _, after = scored_both(ssn, ssn.snap, cfg, jobs, "after the update", state=ssn.snap)
        assert differs(after) >= 1, "the update shows in the oracle's scores"
        ssn.close()


@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_the_calls_change_nothing(gpu, engine):
    snap, cfg = synthetic(300, 2, 70)
    jobs = topology_jobs(snap)
    with T.pkg.KaiCore(cfg) as ca, T.pkg.KaiCore(cfg) as cb:
        sa, sb = ca.open_session(snap), cb.open_session(snap)
        before, stats0 = readback(sa), bytes(sa.stats())
        small = sa.subset_nodes_scored(jobs[:3], engine_path=engine)
        first = sa.subset_nodes_scored(jobs, engine_path=engine)  # (a larger call after a smaller one: the scratch grows)
        assert first[3][:3].tobytes() == small[3].tobytes() and first[4][:3].tobytes() == small[4].tobytes()
        r = T.Result(ans=first[0], sets=first[1], masks=first[2], score_rows=first[3], deciles=first[4])
        pods, ns, rows, so = list_queries(snap, r, jobs)
        one = sa.ordered_nodes_scored(pods[:2], 8, rows, ns[:2], r.score_rows, r.deciles, so[:2])
        more = sa.ordered_nodes_scored(pods, 64, rows, ns, r.score_rows, r.deciles, so)
        assert np.array_equal(more[0][:2, :8], one[0]) and np.array_equal(more[2][:2].clip(max=8), one[2])
        assert_readback_equal(readback(sa), before)
        assert_readback_equal(readback(sa), readback(sb))
        assert bytes(sa.stats()) == stats0, "kai_action_stats_get"
        pending = np.nonzero(sa.pod_states()[0] == abi.POD_STATUS["Pending"])[0][:32]
        na, pa = sa.best_nodes(pending); nb, pb = sb.best_nodes(pending)
        assert np.array_equal(na, nb) and np.array_equal(pa, pb), "best nodes"
        oa, ob = sa.execute("allocate"), sb.execute("allocate")
        assert rows_of(oa) == rows_of(ob) and len(oa) > 0, "the allocate behind the calls against the twin's"
        assert_readback_equal(readback(sa), readback(sb))
        sa.close(); sb.close()


def test_gpu_sessions_the_chip_wide_path_does_not_take(gpu):
    """fraction pods, and quantities that do not add exactly: the engine path, whose scores are still the oracle's.  In the shared-GPU session kai_ordered_nodes_scored with
    k = 1 against single kai_best_node calls: a row with ONE decile orders its nodes as the unscored scan does, so the head is kai_best_node over the nodes that carry it — under
    the spread strategy, where no pre-order range depends on the node set."""
    snap, cfg = synthetic(70, 2, 3)
    synth.add_fractions(snap, 7, frac=0.3)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        _, refs = scored_both(ssn, snap, cfg, topology_jobs(snap), "fractions", want_path=ENGINE, state=snap)
        assert any(r is not None and (r >= 0).any() for r in refs)
        ssn.close()
    spread = abi.default_config(gpu_strategy=abi.SPREAD, cpu_strategy=abi.SPREAD); spread.plugins |= abi.PLUGINS["topology"]
    a = snap.arrays
    D = len(a["domain_parent"])
    with T.pkg.KaiCore(spread) as core:
        ssn = core.open_session(snap)
        pods = np.nonzero(a["pod_status"] == abi.POD_STATUS["Pending"])[0][:24]
        srows = np.zeros(2, R_DT); srows["level_row"] = [0, 1]; srows["n_scored"] = 1
        dec = np.full((2, D), NO_SCORE, np.uint8); dec[0, 1] = 10; dec[1, 2 + 4] = 4  # zone 1; one rack
        keep = [np.nonzero(a["node_domain"][0] == 1)[0], np.nonzero(a["node_domain"][1] == 2 + 4)[0]]
        answered = 0
        for s in (0, 1):
            node, pipe, cnt = ssn.ordered_nodes_scored(pods, 1, None, None, srows, dec, np.full(len(pods), s))
            for t, p in enumerate(pods):
                one = ssn.best_node(int(p), nodeset=keep[s].tolist())
                assert (int(node[t, 0]), bool(pipe[t, 0])) == (int(one[0]), bool(one[1])) or (cnt[t] == 0 and one[0] < 0), (s, t, node[t], one)
                answered += int(cnt[t])
        assert answered > 0
        ssn.close()
    snap, cfg = synthetic(70, 2, 3)
    snap.arrays["node_allocatable"][abi.RES_MEM, 3] += 0.5  # (no integer: the sums are not exact in any order)
    snap.finalize()
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        _, refs = scored_both(ssn, snap, cfg, topology_jobs(snap), "no exact sums", want_path=ENGINE, state=snap)
        assert any(r is not None and (r >= 0).any() for r in refs)
        ssn.close()


def test_gpu_refusals(gpu):
    snap, cfg = synthetic(70, 2, 3)
    jobs = topology_jobs(snap)
    a = snap.arrays
    M, W, D, P = len(jobs), (snap.n_nodes + 31) // 32, len(a["domain_parent"]), snap.n_pods

    def subset(core, cap, version=1, flags=0, q=None, null=()):
        qa = np.zeros(M, Q_DT); qa["job"] = jobs; qa["group"] = -1; qa["podset"] = -1; qa["nodeset"] = -1
        if q is not None: qa[0] = q
        ans = np.full(M * 6, -7, np.int32); sets = np.full(max(cap, 1) * 4, -8, np.int32); maps = np.full(max(cap, 1) * W, 0x99, np.uint32); n = C.c_int64(-3); r = abi.KaiSubsetResult(11, 12, 13)
        sr = np.full(M * 2, -9, np.int32); dec = np.full(M * D, 0x66, np.uint8)
        pm = abi.KaiSubsetParams(version, flags)
        rc = core.lib.kai_subset_nodes_scored(core.handle, C.byref(pm), qa.ctypes.data_as(C.POINTER(abi.KaiSubsetQuery)), M, None, 0, ans.ctypes.data_as(C.POINTER(abi.KaiSubsetAnswer)),
                                              sets.ctypes.data_as(C.POINTER(abi.KaiNodeSet)), cap, C.byref(n), maps.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              None if "score_rows" in null else sr.ctypes.data_as(C.POINTER(abi.KaiTopoScoreRow)), None if "deciles" in null else dec.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(r))
        untouched = bool((ans == -7).all() and (sets == -8).all() and (maps == 0x99).all() and (sr == -9).all() and (dec == 0x66).all() and (r.n_sets, r.path, r.pad) == (11, 12, 13))
        return rc, n.value, untouched

    def ordered(core, qs, k=8, srows=((1, 1), (-1, 0)), dec=None, n_srows=None):
        arr = np.array(list(qs), SQ_DT); sr = np.array(list(srows), R_DT)
        dd = np.full((len(sr), D), NO_SCORE, np.uint8) if dec is None else dec
        out = np.full(len(arr) * max(k, 1) * 2, 0x5a5a5a5a, np.int32); no = np.full(len(arr), 0x5a5a5a5a, np.int32)
        rc = core.lib.kai_ordered_nodes_scored(core.handle, arr.ctypes.data_as(C.POINTER(abi.KaiScoredQuery)), len(arr), None, 0, sr.ctypes.data_as(C.POINTER(abi.KaiTopoScoreRow)),
                                               dd.ctypes.data_as(C.POINTER(C.c_uint8)), len(sr) if n_srows is None else n_srows, k, out.ctypes.data_as(C.POINTER(abi.KaiNodeAnswer)), no.ctypes.data_as(C.POINTER(C.c_int32)))
        return rc, bool((out == 0x5a5a5a5a).all() and (no == 0x5a5a5a5a).all())

    good = [(0, -1, 0, 0), (1, -1, 0, -1), (P - 1, -1, 1, 1)]
    with T.pkg.KaiCore(cfg) as core:
        assert subset(core, 64) == (-6, -3, True) and ordered(core, good) == (-6, True), "KAI_ERR_STATE without an open session"
        ssn = core.open_session(snap)
        before = readback(ssn)
        assert subset(core, 64, version=2) == (-1, -3, True) and subset(core, 64, flags=2) == (-1, -3, True) and subset(core, -1) == (-1, -3, True)
        assert subset(core, 64, q=(snap.n_jobs, -1, -1, -1)) == (-1, -3, True) and subset(core, 64, null=("score_rows",)) == (-1, -3, True) and subset(core, 64, null=("deciles",)) == (-1, -3, True)
        total = len(ssn.subset_nodes(jobs)[1])
        for flags in (0, abi.SUBSET_ENGINE_PATH):
            assert subset(core, total - 1, flags=flags) == (-4, total, True), "KAI_ERR_CAPACITY: *n_sets_out holds the number needed, every other output untouched"
            assert subset(core, total, flags=flags)[:2] == (0, total)
        d11 = np.full((2, D), NO_SCORE, np.uint8); d11[1, D - 1] = 11
        for bad in (dict(qs=good + [(0, -1, 0, 2)]), dict(qs=good + [(0, -1, 0, -2)]), dict(qs=good + [(P, -1, 0, -1)]), dict(qs=good + [(0, 0, 0, -1)]), dict(qs=good + [(0, -1, 2, -1)]), dict(qs=good, k=0),
                    dict(qs=good, k=65), dict(qs=good, n_srows=-1), dict(qs=good, srows=((a["node_domain"].shape[0], 0), (-1, 0))), dict(qs=good, srows=((-3, 0), (-1, 0))), dict(qs=good, dec=d11)):
            assert ordered(core, **bad) == (-1, True), bad
        assert ordered(core, good)[0] == 0
        assert_readback_equal(readback(ssn), before)
        ssn.close()
    with T.pkg.KaiCore(cfg, world=2, rank=0, allgather=lambda send, recv, nbytes: 1) as grp:
        assert subset(grp, 64) == (-5, -3, True) and ordered(grp, good) == (-5, True), "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
