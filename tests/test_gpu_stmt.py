"""kai_stmt_* on the MI355X, through the C ABI (Session.statement()).  Operations and expected states come from the oracle — its Statement scripts
(tests/test_oracle_statement.py run_script) and T.Oracle.run — never from the code under test: behind every call pod states, node states and queue shares must be the
oracle's or a twin handle's, bit for bit, on the chip-wide path and on the engine walk.  The same cases at the same sizes run with emulated lanes in tests/test_stmt.py;
the composed walk — kai_subset_nodes, kai_ordered_nodes, apply, rollback, commit — included."""
import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import crowded, gpu  # noqa: F401  (fixture)
from test_gpu_ops_apply import read, rows, same
import test_ops_apply as OA
import test_stmt as TS

pytestmark = pytest.mark.gpu
abi = T.abi
S = abi.POD_STATUS
ALLOCATE, PIPELINE, EVICT, WIDE, ENGINE = TS.ALLOCATE, TS.PIPELINE, TS.EVICT, TS.WIDE, TS.ENGINE


def same_oracle(ssn, snap, cfg, rows_, what):
    _, st, nd, nodes = TS.oracle_state(snap, cfg, rows_)
    OA.same_state(read(ssn), np.array(st, np.int32), np.array(nd, np.int32), nodes, what=what)


def play(stmt, sc, steps, k, engine):
    st = steps[k]
    if st[0] == "apply": return stmt.apply(OA.make_ops(sc[st[1]:st[2]]), engine_path=engine)
    if st[0] == "rollback": return stmt.rollback(st[1], engine_path=engine)
    return stmt.discard(engine_path=engine)


# ---- (3) the oracle's Statement scripts
def test_gpu_statement_scripts_against_the_oracle(gpu):
    """every script of tests/test_ops_apply.py script_sessions() in every shape of tests/test_stmt.py script_shapes(): behind every call the oracle's Statement's pod status and
    node and node Idle / Releasing / Used (Allocated against Allocated: nothing is committed), on both paths; the two paths agree in the shares too"""
    n_calls = 0
    for name, snap, cfg, scripts in OA.script_sessions():
        with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
            sa, sb = a.open_session(snap), b.open_session(snap)
            for i, sc in enumerate(scripts):
                for shape, steps in TS.script_shapes(sc):
                    sa.reset(); sb.reset()
                    ta, tb = sa.statement(), sb.statement()
                    once = len({p for _, p, _ in sc}) == len(sc)  # every pod once, from Pending / Running: every call is the chip-wide path's
                    for k in range(len(steps)):
                        ra, rb = play(ta, sc, steps, k, False), play(tb, sc, steps, k, True)
                        assert rb.path == ENGINE and (ra.path == WIDE if once else ra.path in (WIDE, ENGINE)) and ra.log_len == rb.log_len, (name, i, shape, k, ra.path)
                        same_oracle(sa, snap, cfg, TS._prefix_rows(sc, steps, k), f"{name}-{i}-{shape} step {k}")
                        same(read(sa), read(sb), f"{name}-{i}-{shape} step {k}: against the engine path")
                        n_calls += 1
                    if steps[-1][0] != "discard": ta.discard(); tb.discard()
            sa.close(); sb.close()
    assert n_calls > 100


def test_gpu_the_paths_take_over_from_each_other(gpu):
    """chip-wide batches, then a batch that names two pods of the log again (the engine takes it), rolled back across the seam; and a batch the engine is made to take with a
    chip-wide batch behind it, rolled back one by one — every state against the oracle's Statement"""
    snap, cfg, once, again, more = TS.config0_batches()
    sc = once + again + more; a, b, n = len(once), len(once) + len(again), len(once) + len(again) + len(more)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        fresh = read(ssn)
        steps = [("apply", 0, a), ("apply", a, b), ("apply", b, n), ("rollback", b), ("rollback", 3), ("apply", 3, a), ("discard",)]
        t = ssn.statement(); paths = []
        for k in range(len(steps)):
            paths.append(play(t, sc, steps, k, False).path)
            same_oracle(ssn, snap, cfg, TS._prefix_rows(sc, steps, k), f"wide then engine: step {k}")
        assert paths == [WIDE, ENGINE, WIDE, WIDE, ENGINE, WIDE, WIDE], paths
        same(read(ssn), fresh, "the discard restores the read-backs")
        t = ssn.statement()
        assert t.apply(OA.make_ops(sc[:a]), engine_path=True).path == ENGINE and t.apply(OA.make_ops(sc[b:])).path == WIDE
        assert t.rollback(a).path == WIDE and t.apply(OA.make_ops(sc[b:])).path == WIDE
        assert t.rollback(2).path == ENGINE
        same_oracle(ssn, snap, cfg, [(OA.TO_ORACLE[k], p, nd, 1) for k, p, nd in sc[:2]], "engine then wide: rolled back to 2")
        assert t.discard().path == ENGINE
        same(read(ssn), fresh, "the discard restores the read-backs")
        ssn.close()


# ---- (4) plugins on, exact sums
@pytest.fixture(scope="module")
def allocate_case():
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    return snap, cfg, T.Oracle.run(snap, cfg, ("allocate",))


@pytest.mark.parametrize("engine", [False, True], ids=["wide", "engine"])
def test_gpu_allocate_in_chunks_rollbacks_discard_commit(gpu, allocate_case, engine):
    """the oracle's allocate (649 operations) in chunks with checkpoints at 1, 63, 64, 65 and 257 operations; rolled back to each: the read-backs of a twin handle that
    applied only that prefix; discard: the fresh read-backs; commit of the whole action: the oracle's state and kai_ops_apply's on the twin; the allocate action afterwards:
    the twin's operations and batch-path count"""
    snap, cfg, ref = allocate_case
    n = len(ref.ops); assert n == 649
    ops = OA.ref_ops(ref); ops["stmt"] = 0
    want = ENGINE if engine else WIDE
    edges = [0] + TS.CUTS + [n]
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        fresh = read(sa)
        t = sa.statement()
        for i in range(len(edges) - 1):
            assert t.checkpoint() == edges[i]
            r = t.apply(ops[edges[i]:edges[i + 1]], engine_path=engine)
            assert (r.path, r.log_len, r.first_bad) == (want, edges[i + 1], -1)
        st = ref.pod_status.copy(); st[st == S["Binding"]] = S["Allocated"]  # nothing is committed
        OA.same_state(read(sa), st, ref.pod_node, ref.nodes, ref.shares_final, "the whole action, uncommitted")
        for cp in reversed(TS.CUTS):
            r = t.rollback(cp, engine_path=engine)
            assert (r.path, r.log_len) == (want, cp)
            sb.reset(); tb = sb.statement(); tb.apply(ops[:cp], engine_path=engine)
            same(read(sa), read(sb), f"rolled back to {cp} against the twin")
        assert t.discard(engine_path=engine).log_len == 0
        same(read(sa), fresh, "discard")
        # commit of the whole action, with a rollback on the way
        sb.reset()
        t = sa.statement()
        t.apply(ops[:300], engine_path=engine); t.apply(ops[300:], engine_path=engine); t.rollback(300, engine_path=engine); t.apply(ops[300:], engine_path=engine)
        got, r = t.commit()
        assert r.path == want and rows(got) == ref.ops and (got["stmt"] == 0).all() and got["seq"].tolist() == list(range(n))
        same(read(sa), ref, "committed")
        rb = sb.apply_ops(ops, engine_path=engine)
        assert rb.path == want
        same(read(sa), read(sb), "commit against kai_ops_apply")
        xa, xb = rows(sa.execute("allocate")), rows(sb.execute("allocate"))
        assert xa == xb and sa.stats().reserved[4] == sb.stats().reserved[4]
        same(read(sa), read(sb), "the allocate action behind the commit")
        # ... and behind the commit of a prefix, where the action still finds pods to place
        sa.reset(); sb.reset()
        t = sa.statement()
        t.apply(ops[:300], engine_path=engine); t.rollback(257, engine_path=engine)
        got, r = t.commit()
        assert rows(got) == ref.ops[:257]
        sb.apply_ops(ops[:257], engine_path=engine)
        same(read(sa), read(sb), "commit of a prefix against kai_ops_apply")
        xa, xb = rows(sa.execute("allocate")), rows(sb.execute("allocate"))
        assert xa == xb and len(xa) > 0 and sa.stats().reserved[4] == sb.stats().reserved[4]
        same(read(sa), read(sb), "the allocate action behind the commit of a prefix")
        sa.close(); sb.close()


@pytest.mark.parametrize("seed,action,counts", OA.WIDE_VICTIM, ids=[f"crowded{s}-{a}" for s, a, _ in OA.WIDE_VICTIM])
def test_gpu_evictions_and_pipelines(gpu, seed, action, counts):
    """a victim action's operations (evictions, pipelines, allocations) applied, rolled back to the middle and to nothing, applied again, committed: the oracle's state; rolled
    back evictions do not keep the next allocate off its batch path, committed ones do, as on the kai_ops_apply twin"""
    snap, cfg = crowded(seed)
    ref = T.Oracle.run(snap, cfg, (action,))
    n = len(ref.ops); m = n // 2
    ops = OA.ref_ops(ref); ops["stmt"] = 0
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        fresh = read(sa)
        for engine in (False, True):
            want = ENGINE if engine else WIDE
            sa.reset(); sb.reset()
            t = sa.statement()
            assert t.apply(ops[:m], engine_path=engine).path == want
            mid = read(sa)
            assert t.apply(ops[m:], engine_path=engine).path == want
            assert t.rollback(m, engine_path=engine).path == want
            same(read(sa), mid, "rolled back to the middle")
            assert t.rollback(0, engine_path=engine).path == want
            same(read(sa), fresh, "rolled back to nothing")
            t.apply(ops, engine_path=engine)
            got, r = t.commit()
            assert r.path == want and rows(got) == ref.ops
            same(read(sa), ref, "committed")
            sb.apply_ops(ops, engine_path=engine)
            same(read(sa), read(sb), "commit against kai_ops_apply")
            assert rows(sa.execute("allocate")) == rows(sb.execute("allocate")) and sa.stats().reserved[4] == sb.stats().reserved[4]
            # everything rolled back, nothing committed: the allocate action of an untouched twin
            sa.reset(); sb.reset()
            t = sa.statement(); t.apply(ops, engine_path=engine); t.discard(engine_path=engine)
            assert rows(sa.execute("allocate")) == rows(sb.execute("allocate")) and sa.stats().reserved[4] == sb.stats().reserved[4]
            same(read(sa), read(sb), "allocate behind a discarded Statement")
        sa.close(); sb.close()


# ---- (5) a precondition that fails in the middle of a Statement
def test_gpu_a_failing_precondition_leaves_the_statement_as_it_was(gpu, allocate_case):
    snap, cfg, ref = allocate_case
    st, nd = snap.arrays["pod_status"], snap.arrays["pod_node"]
    used = {o[1] for o in ref.ops}
    running = [int(p) for p in np.nonzero((st == S["Running"]) & (nd >= 0))[0] if p not in used]
    good = list(ref.ops)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        for engine in (False, True):
            ssn.reset()
            t = ssn.statement()
            t.apply(OA.make_ops(good[:100]), engine_path=engine)
            before = read(ssn)
            for batch, bad in ((good[100:120] + [(ALLOCATE, running[0], 0)] + good[120:140], 20),      # a Running pod allocated: the check finds it
                               (good[120:140] + [good[5]] + good[140:150], 20),                        # a pod of the log allocated again: the walk over the shadow finds it
                               (good[140:150] + [(EVICT, good[150][1], good[150][2])], 10)):           # a Pending pod evicted
                with pytest.raises(T.pkg.core.KaiError) as e:
                    t.apply(OA.make_ops(batch), engine_path=engine)
                assert e.value.code == -6 and e.value.result.first_bad == bad and e.value.result.log_len == 100, (e.value.code, e.value.result.first_bad)
                same(read(ssn), before, "a refused batch writes nothing")
                assert t.checkpoint() == 100
            t.apply(OA.make_ops(good[100:120]), check_only=True, engine_path=engine)
            same(read(ssn), before, "check only writes nothing"); assert t.checkpoint() == 100
            t.rollback(50, engine_path=engine)
            r = t.apply(OA.make_ops(good[50:100]), engine_path=engine)
            assert r.log_len == 100 and r.path == (ENGINE if engine else WIDE), "pods that were rolled back are allocated again, on the chip-wide path"
            same(read(ssn), before, "applied again")
            t.discard()
        ssn.close()


# ---- (6) queries while a Statement is open
def test_gpu_queries_see_the_tentative_state_and_leave_the_log(gpu):
    """best_nodes and ordered_nodes over all Pending pods, job_order and subset_nodes on both their paths while a Statement is open: the answers of a twin that took the same
    operations through kai_ops_apply; afterwards the log is what it was — a rollback restores the fresh read-backs, the checkpoint has not moved"""
    import test_subset_nodes as SN
    snap, cfg = SN.synthetic(48, 2, 3)
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    n = min(len(ref.ops), 40); assert n >= 8
    ops = OA.ref_ops(ref, 0, n); ops["stmt"] = 0
    jobs = SN.topology_jobs(snap)

    def ask(ssn):
        st, _ = ssn.pod_states()
        pend = np.nonzero(st == S["Pending"])[0]
        out = [ssn.best_nodes(pend), ssn.ordered_nodes(pend, 4)]
        for ep in (False, True):
            o = ssn.job_order(depth=-1, engine_path=ep); out.append((o[0], o[1], o[2], o[3].path))
            s = ssn.subset_nodes(jobs, engine_path=ep); out.append((s[0], s[1], s[2], s[3].path))
        return out

    def equal(x, y):
        if isinstance(x, (tuple, list)): return len(x) == len(y) and all(equal(a, b) for a, b in zip(x, y))
        return np.array_equal(x, y)

    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        fresh, fresh_answers = read(sa), ask(sa)
        for engine in (False, True):
            sa.reset(); sb.reset()
            t = sa.statement(); t.apply(ops, engine_path=engine)
            sb.apply_ops(ops, engine_path=engine)
            before = read(sa)
            got, want = ask(sa), ask(sb)
            for k in range(len(want)): assert equal(got[k], want[k]), f"query {k} while the Statement is open"
            assert not equal(got, fresh_answers), "the applied operations change an answer (else this test shows nothing)"
            same(read(sa), before, "the queries write nothing"); assert t.checkpoint() == n
            t.rollback(0, engine_path=engine)
            same(read(sa), fresh, "the rollback behind the queries")
            assert equal(ask(sa), fresh_answers)
            t.discard()
        sa.close(); sb.close()


# ---- (7) the walk the feature exists for
def test_gpu_the_composed_walk(gpu):
    """begin; per node set of kai_subset_nodes a checkpoint; per task kai_ordered_nodes(k = 1) inside the set and apply; on an empty answer rollback and the next set; commit.
    The first set (rack A) takes the CPU-only task and has no node for the 3-GPU task: one operation is rolled back.  The end: the oracle's operations and state, and what
    kai_action_execute(allocate) gives on a second handle."""
    snap, cfg = TS.walk_scene()
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    assert ref.ops == TS.WALK_OPS and ref.stats.rollbacks >= 1, "the scene: the oracle rolls back and places both pods in rack B"
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        with sa.statement() as t:
            ans, sets, masks, _ = sa.subset_nodes([0])
            assert ans["status"][0] == 0 and ans["n_sets"][0] == 2
            rolled_back, placed = [], False
            for s in range(int(ans["first"][0]), int(ans["first"][0] + ans["n_sets"][0])):
                cp = t.checkpoint(); placed = True
                for pod in (0, 1):
                    node, pipe, cnt = sa.ordered_nodes([pod], 1, nodesets=[masks[s]], nodeset_of=[0])
                    if cnt[0] == 0: placed = False; break
                    op = np.zeros(1, OA.OP_DT); op["kind"], op["pod"], op["node"] = (PIPELINE if pipe[0, 0] else ALLOCATE), pod, node[0, 0]
                    t.apply(op)
                if placed: break
                rolled_back.append(t.checkpoint() - cp); t.rollback(cp)
            assert placed and rolled_back == [1], rolled_back
            got, r = t.commit()
        assert rows(got) == ref.ops and r.path == WIDE
        same(read(sa), ref, "the walk against the oracle")
        assert rows(sb.execute("allocate")) == ref.ops
        same(read(sa), read(sb), "the walk against kai_action_execute(allocate)")
        sa.close(); sb.close()
