"""kai_stmt_place on the MI355X, through the C ABI (Statement.place).  Every case runs the loop the contract names — checkpoint; per task kai_ordered_nodes_scored(k = 1) and
kai_stmt_apply of one operation; kai_stmt_rollback of a set that fails — on a twin handle and compares answers, fail_at, operations, the three read-backs and what later
rollbacks, commits and actions give; where the scene is the allocate action's, also with the oracle.  The same scenes run with emulated lanes in tests/test_stmt_place.py."""
import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import crowded, gpu  # noqa: F401  (fixture)
from test_gpu_ops_apply import read, rows, same
import test_ops_apply as OA
import test_stmt as TS
import test_stmt_place as SP
import test_subset_nodes as SN
import test_topo_scores as TSC

pytestmark = pytest.mark.gpu
abi = T.abi
S = abi.POD_STATUS
ALLOCATE, PIPELINE, EVICT, WIDE, ENGINE = TS.ALLOCATE, TS.PIPELINE, TS.EVICT, TS.WIDE, TS.ENGINE
PLACED, NO_FIT = abi.PLACE_PLACED, abi.PLACE_NO_FIT


def the_loop(ssn, t, gangs, nodesets=None, score_rows=None, deciles=None, pipeline_only=False, engine_path=False):
    """the loop of kai_stmt_place's contract over the existing calls -> (answers as tuples (status, set, sets_tried, first_op, n_ops), fail_at per gang, operations as
    (kind, pod, node, job, seq))"""
    len0 = t.checkpoint()
    answers, fails, ops = [], [], []
    for gang in gangs:
        pods, sets, scores = list(gang[0]), list(gang[1]), (gang[2] if len(gang) > 2 else -1)
        cp = t.checkpoint()
        took, tried, fail_at = -1, 0, [-1] * len(sets)
        for si, s in enumerate(sets):
            tried += 1; fail = len(pods)
            for ti, p in enumerate(pods):
                kw = dict(nodesets=[nodesets[s]], nodeset_of=[0]) if s is not None and s >= 0 else {}
                node, pipe, cnt = ssn.ordered_nodes_scored([p], 1, score_rows=score_rows, deciles=deciles, scores_of=[scores], pipeline_only=pipeline_only, **kw)
                if cnt[0] == 0: fail = ti; break
                op = np.zeros(1, OA.OP_DT); op["kind"], op["pod"], op["node"] = (PIPELINE if pipe[0, 0] else ALLOCATE), p, node[0, 0]
                r = t.apply(op, engine_path=engine_path)
                ops.append((int(op["kind"][0]), int(p), int(node[0, 0]), int(ssn.snap.arrays["pod_job"][p]), r.log_len - 1))
            fail_at[si] = fail
            if fail == len(pods): took = si; break
            t.rollback(cp, engine_path=engine_path); del ops[cp - len0:]
        answers.append((PLACED if took >= 0 else NO_FIT, took, tried, cp - len0, t.checkpoint() - cp)); fails.append(fail_at)
    return answers, fails, ops


def one_call(t, gangs, **kw):
    ans, fail, ops, res = t.place(gangs, **kw)
    return [tuple(int(x) for x in (a["status"], a["set"], a["sets_tried"], a["first_op"], a["n_ops"])) for a in ans], [f.tolist() for f in fail], \
        [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["seq"])) for o in ops], res


def both(sa, sb, ta, tb, gangs, what, engine=False, **kw):
    """one call on handle a, the loop on its twin b: the same outputs, log length and read-backs"""
    got = one_call(ta, gangs, engine_path=engine, **kw)
    want = the_loop(sb, tb, gangs, engine_path=engine, **kw)
    assert got[0] == want[0], f"{what}: answers {got[0]} / {want[0]}"
    assert got[1] == want[1], f"{what}: fail_at {got[1]} / {want[1]}"
    assert got[2] == want[2], f"{what}: operations {got[2]} / {want[2]}"
    assert got[3].log_len == tb.checkpoint() == ta.checkpoint(), what
    same(read(sa), read(sb), f"{what}: against the loop over the existing calls")
    return got


def twins(snap, cfg):
    a, b = T.pkg.KaiCore(cfg), T.pkg.KaiCore(cfg)
    return a, b, a.open_session(snap), b.open_session(snap)


# ---- (2) the scene of the composed walk
@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_the_walks_scene_in_one_call(gpu, engine):
    snap, cfg = TS.walk_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    assert ref.ops == TS.WALK_OPS
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b, T.pkg.KaiCore(cfg) as c:
        sa, sb, sc = a.open_session(snap), b.open_session(snap), c.open_session(snap)
        ans, _, masks, _ = sa.subset_nodes([0])
        assert ans["n_sets"][0] == 2
        ta, tb = sa.statement(), sb.statement()
        got = both(sa, sb, ta, tb, [([0, 1], [0, 1])], "the walk's scene", engine=engine, nodesets=[masks[0], masks[1]])
        assert got[0] == [(PLACED, 1, 2, 0, 2)] and got[1] == [[1, 2]] and [o[:4] for o in got[2]] == TS.WALK_OPS and got[3].path == (ENGINE if engine else WIDE)
        oa, ra = ta.commit(); ob, _ = tb.commit()
        assert rows(oa) == ref.ops == rows(ob) and ra.path == (ENGINE if engine else WIDE)
        same(read(sa), ref, "one call and a commit against the oracle")
        assert rows(sc.execute("allocate")) == ref.ops
        same(read(sa), read(sc), "one call and a commit against kai_action_execute(allocate)")
        assert rows(sa.execute("allocate")) == rows(sc.execute("allocate")) and sa.stats().reserved[4] == sc.stats().reserved[4]
        sa.close(); sb.close(); sc.close()


# ---- (3) state dependence inside a gang, (4) a gang no set takes
@pytest.mark.parametrize("N", [48, 70])
def test_gpu_a_task_sees_what_its_predecessors_took(gpu, N):
    snap, cfg, pend = SP.binpack_scene(N)
    gang = pend[:10]
    first = [o[2] for o in T.Oracle.run(snap, cfg, ("allocate",)).ops if o[1] == gang[0]]
    big = [n for n in range(N) if n not in (0, 31, 64)]
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        fresh = read(sa)
        entry, _, cnt = sa.ordered_nodes(gang, 1, nodesets=[big], nodeset_of=[0] * len(gang))
        for engine in (False, True):
            sa.reset(); sb.reset()
            ta, tb = sa.statement(), sb.statement()
            got = both(sa, sb, ta, tb, [(gang, [0, 1])], f"bin-pack, {N} nodes", engine=engine, nodesets=[first, big])
            assert got[0][0][:3] == (PLACED, 1, 2) and 1 <= got[1][0][0] < len(gang) and got[1][0][1] == len(gang)
            nodes = [o[2] for o in got[2]]
            assert len(set(nodes)) > 1 and any(x != y for x, y in zip(nodes, entry[:, 0].tolist())), "a task's node differs from the entry state's answer (else the scene shows nothing)"
            # a gang no set takes: nothing is left, and kai_stmt_apply of its pods afterwards is the chip-wide path's
            mid = read(sa); n = ta.checkpoint()
            rest = [p for p in pend if p not in gang]  # all the other pods the session has room for, on ONE node: they do not fit
            got = both(sa, sb, ta, tb, [(rest, [0, 0])], "a gang no set takes", engine=engine, nodesets=[first, big])
            assert got[0] == [(NO_FIT, -1, 2, 0, 0)] and got[2] == [] and got[3].log_len == n
            same(read(sa), mid, "a gang no set takes: the read-backs as before the call")
            nd, _, cnt2 = sa.ordered_nodes(rest[:1], 1)
            op = np.zeros(1, OA.OP_DT); op["kind"], op["pod"], op["node"] = ALLOCATE, rest[0], nd[0, 0]
            assert cnt2[0] == 1 and ta.apply(op).path == WIDE and tb.apply(op).path == WIDE
            for cp in (n, 3, 0):
                assert ta.rollback(cp, engine_path=engine).log_len == tb.rollback(cp, engine_path=engine).log_len == cp
                same(read(sa), read(sb), f"rolled back to {cp}")
            same(read(sa), fresh, "everything rolled back")
            ta.discard(); tb.discard()
        sa.close(); sb.close()


# ---- (5) three gangs in one call, the middle one failing on its queue's limit
@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_three_gangs_the_middle_one_fails(gpu, engine):
    snap, cfg = SP.limit_scene()
    a, b, sa, sb = twins(snap, cfg)
    with a, b:
        ta, tb = sa.statement(), sb.statement()
        got = both(sa, sb, ta, tb, [([0, 1], [0]), ([2, 3, 4], [1, -1]), ([5], [-1])], "three gangs", engine=engine, nodesets=[(0, 1), (2, 3)])
        assert got[0] == [(PLACED, 0, 1, 0, 2), (NO_FIT, -1, 2, 2, 0), (PLACED, 0, 1, 2, 1)] and got[1] == [[2], [1, 1], [1]]
        assert [o[1] for o in got[2]] == [0, 1, 5] and [o[4] for o in got[2]] == [0, 1, 2]
        oa, _ = ta.commit(); ob, _ = tb.commit()
        assert rows(oa) == rows(ob)
        same(read(sa), read(sb), "committed")
        sa.close(); sb.close()


# ---- (6) pipelines
@pytest.mark.parametrize("seed,action,counts", OA.WIDE_VICTIM, ids=[f"crowded{s}-{a}" for s, a, _ in OA.WIDE_VICTIM])
def test_gpu_tasks_placed_on_released_room_are_pipelined(gpu, seed, action, counts):
    snap, cfg = crowded(seed)
    ref = T.Oracle.run(snap, cfg, (action,))
    ev = OA.make_ops([o for o in ref.ops if o[0] == EVICT]); pods = [o[1] for o in ref.ops if o[0] == PIPELINE]
    gangs = [([p], [-1]) for p in pods]
    a, b, sa, sb = twins(snap, cfg)
    with a, b:
        seen = False
        for engine in (False, True):
            for po in (False, True):
                sa.reset(); sb.reset()
                ta, tb = sa.statement(), sb.statement()
                ta.apply(ev, engine_path=engine); tb.apply(ev, engine_path=engine)
                got = both(sa, sb, ta, tb, gangs, f"pipelines, only {po}", engine=engine, pipeline_only=po)
                kinds = [o[0] for o in got[2]]
                seen = seen or PIPELINE in kinds
                if po: assert kinds and all(k == PIPELINE for k in kinds)
                assert [o[4] for o in got[2]] == list(range(len(ev), len(ev) + len(kinds)))
                oa, _ = ta.commit(); ob, _ = tb.commit()
                assert rows(oa) == rows(ob)
                same(read(sa), read(sb), "committed")
                assert rows(sa.execute("allocate")) == rows(sb.execute("allocate")) and sa.stats().reserved[4] == sb.stats().reserved[4]
        assert seen, "no task was pipelined: the scene shows nothing"
        sa.close(); sb.close()


# ---- (7) scores
@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_a_scored_gang_lands_where_the_allocate_action_puts_it(gpu, engine):
    snap, cfg = TSC.gang_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    gang = snap.job_names.index("gang")
    mine = [o for o in ref.ops if o[3] == gang]
    a, b, sa, sb = twins(snap, cfg)
    with a, b:
        ans, sets, masks, score_rows, deciles, _ = sa.subset_nodes_scored([gang])
        assert ans["n_sets"][0] == 1 and score_rows["level_row"][0] == 1
        pods = [o[1] for o in mine]
        ta, tb = sa.statement(), sb.statement()
        got = both(sa, sb, ta, tb, [(pods, [0], 0)], "the scored gang", engine=engine, nodesets=[masks[0]], score_rows=score_rows, deciles=deciles)
        assert [o[:4] for o in got[2]] == mine, "pod for pod where the oracle's allocate puts the gang"
        ta.rollback(0); tb.rollback(0)
        plain = one_call(ta, [(pods, [0])], nodesets=[masks[0]], engine_path=engine)
        assert plain[2][0][2] != mine[0][2], "without the score row the gang starts elsewhere (else the scores show nothing)"
        ta.discard(); tb.discard()
        sa.close(); sb.close()


# ---- (8) seams
@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_the_calls_records_and_kai_stmt_applys_lie_on_one_log(gpu, engine):
    snap, cfg, pend = SP.binpack_scene(48)
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    under = [o for o in ref.ops if o[0] == ALLOCATE][:5]
    used = {o[1] for o in under}
    free = [p for p in pend if p not in used]
    gangs = [(free[0:3], [0, -1]), (free[3:5], [-1]), (free[5:9], [1, 0, -1])]
    nodesets = [list(range(5, 40)), [2, 3]]
    over = OA.make_ops([(PIPELINE, free[9], 3), (ALLOCATE, free[10], 4)])
    a, b, sa, sb = twins(snap, cfg)
    with a, b:
        for rb in (False, True):
            sa.reset(); sb.reset()
            ta, tb = sa.statement(), sb.statement()
            ta.apply(OA.make_ops(under), engine_path=engine); tb.apply(OA.make_ops(under), engine_path=engine)
            got = both(sa, sb, ta, tb, gangs, "over kai_stmt_apply's records", engine=engine, nodesets=nodesets)
            n = ta.checkpoint()
            assert n > 5 + 3 and got[3].path == (ENGINE if engine else WIDE)
            ta.apply(over, engine_path=engine); tb.apply(over, engine_path=engine)
            for cp in (n + 1, n - 1, 6, 5, 2):
                ra, rbb = ta.rollback(cp, engine_path=rb), tb.rollback(cp, engine_path=rb)
                assert ra.log_len == rbb.log_len == cp and ra.path == rbb.path and (ra.path == WIDE or engine or rb), (cp, ra.path, rbb.path)
                same(read(sa), read(sb), f"rolled back to {cp}")
            got = both(sa, sb, ta, tb, gangs[:2], "again, over the rest", engine=engine, nodesets=nodesets)
            oa, ra = ta.commit(); ob, rbb = tb.commit()
            assert rows(oa) == rows(ob) and ra.path == rbb.path and oa["seq"].tolist() == list(range(len(oa)))
            same(read(sa), read(sb), "committed")
            assert rows(sa.execute("allocate")) == rows(sb.execute("allocate")) and sa.stats().reserved[4] == sb.stats().reserved[4]
            same(read(sa), read(sb), "the allocate action behind the commit")
        sa.close(); sb.close()


def test_gpu_a_pod_that_is_not_pending_refuses_the_call(gpu):
    snap, cfg, pend = SP.binpack_scene(48)
    running = int(np.nonzero(snap.arrays["pod_status"] == S["Running"])[0][0])
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        for engine in (False, True):
            t = ssn.statement()
            t.apply(OA.make_ops([(ALLOCATE, pend[5], int(T.Oracle.run(snap, cfg, ("allocate",)).pod_node[pend[5]]))]))
            before = read(ssn)
            for gangs, bad in (([(pend[:3], [-1]), ([pend[3], running, pend[4]], [-1])], 4), ([([pend[0], pend[5]], [-1])], 1)):  # a Running pod; a pod the Statement allocated
                with pytest.raises(T.pkg.core.KaiError) as e:
                    t.place(gangs, engine_path=engine)
                assert e.value.code == -6 and e.value.result.first_bad == bad and e.value.result.log_len == 1
                same(read(ssn), before, "a refused call writes nothing"); assert t.checkpoint() == 1
            with pytest.raises(T.pkg.core.KaiError) as e:
                t.place([([pend[0], pend[0]], [-1])])
            assert e.value.code == -1
            ans, _, ops, r = t.place([(pend[:2], [-1])], engine_path=engine)
            assert r.log_len == 3 and len(ops) == 2 and ops["seq"].tolist() == [1, 2]
            t.discard()
        ssn.close()


# ---- (9) a whole action composed
@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_a_whole_allocate_action_in_one_call(gpu, engine):
    """kai_job_order, one kai_subset_nodes_scored, one kai_stmt_place over all jobs, commit: the oracle's allocate"""
    snap, cfg = SP.action_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    a, b, sa, sb = twins(snap, cfg)
    with a, b:
        order = sa.job_order(depth=-1)[0].tolist()
        seq = SP.oracle_job_sequence(ref)
        assert [j for j in order if j in seq] == seq and len(order) == 5, "one leaf queue: the pop order at the entry state is the action's"
        ans, sets, masks, score_rows, deciles, _ = sa.subset_nodes_scored(order)
        gangs = [(SP.pending_pods(snap, j), list(range(int(ans["first"][i]), int(ans["first"][i] + ans["n_sets"][i]))), i) for i, j in enumerate(order) if ans["status"][i] == 0 and ans["n_sets"][i] > 0]
        assert len(gangs) == 4
        ta, tb = sa.statement(), sb.statement()
        got = both(sa, sb, ta, tb, gangs, "the composed action", engine=engine, nodesets=list(masks), score_rows=score_rows, deciles=deciles)
        assert [x[0] for x in got[0]] == [PLACED, PLACED, PLACED, NO_FIT] and got[0][3][2] == 3
        assert [o[:4] for o in got[2]] == ref.ops, "the (kind, pod, node, job) sequence is the oracle's allocate"
        oa, _ = ta.commit(); tb.commit()
        assert rows(oa) == ref.ops
        same(read(sa), ref, "the composed action against the oracle")
        sa.close(); sb.close()
