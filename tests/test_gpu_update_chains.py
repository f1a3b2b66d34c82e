"""kai_session_update / kai_session_update_rows across CHAINS of updates on the MI355X (tests/update_chains.py): one handle A opens S_0 and lives for the whole
chain; after every update it must be indistinguishable from a fresh handle that opens S_k with cfg_k — the same read-backs bit for bit, the same operations, Statement
ids, decision counters and path from the cycle that follows — and the cycle must be the oracle's on (S_k, cfg_k), which is also the cycle the chain was built from
on the CPU (tests/test_update_chains.py): the device is the runner here, and every element it produces is compared with the oracle-built chain's before it is used.
A step without rows goes through kai_session_update, one with rows through kai_session_update_rows.  Between a cycle and the next update the chain asks for a
kai_session_reset (back to S_k, compared with the fresh handle's) or for kai_best_nodes / kai_ordered_nodes over the pods still pending, on both handles.

The random chains have a follower F as well: it opens S_0, never executes an action, takes A's operations of every cycle through kai_ops_apply (one call per action)
— its read-back then equals A's after the cycle — and then the same update; after the last update it runs the cycle itself, which must equal the fresh handle's.
(kai_ops_apply refuses a session with shared-GPU requests, so the shared-GPU seeds run without F.)  At most three handles are live at once."""
import numpy as np
import pytest

import kai_testlib as T
import update_chains as U
from test_engine_hostsim import _same_groups
from test_gpu_parity import assert_same, assert_same_tol, gpu  # noqa: F401  (fixture)
from test_gpu_session_update import assert_cycle_equal, assert_readback_equal, readback

pytestmark = pytest.mark.gpu
pkg = T.pkg
abi = pkg.abi


def cycle(ssn, actions):
    """test_gpu_session_update.run_cycle, keeping each action's kai_op array for kai_ops_apply: (arrays, (operations, counters and path, read-back))."""
    raw, ops, stats = [], [], []
    for a in actions:
        arr = ssn.execute(a)
        raw.append(arr)
        ops += [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["stmt"])) for o in arr]
        s = ssn.stats()
        stats.append((s.decisions, s.jobs_attempted, s.jobs_committed, s.rollbacks, s.reserved[4] != 0))
    return raw, (ops, stats, readback(ssn))


def as_result(raw, run, opened):
    """A cycle as T.Oracle.run reports one: the Statement ids numbered through the cycle (kai_op.stmt counts from 0 in every action)."""
    stmts = []
    for arr in raw:
        base = (stmts[-1] + 1) if stmts else 0
        stmts += [int(o["stmt"]) + base for o in arr]
    rb = run[2]
    return T.Result(ops=[o[:4] for o in run[0]], stmts=stmts, pod_status=rb["status"], pod_node=rb["node"], gpu_groups=rb["groups"], shares_open=opened["shares"],
                    shares_final=rb["shares"], nodes=rb["nodes"])


def update(ssn, it):
    if it.rows is None:
        ssn.update(**it.delta)
    else:
        ssn.update_rows(it.delta, it.rows)


def walk(key, follower=False):
    ref = U.oracle_chain(key)
    spec = U.RandomChain(key) if isinstance(key, int) else getattr(U, key)()
    actions = spec.actions
    live = {"A": None, "B": None, "F": None}  # the cores: the handle under test, the fresh one of the current step, the follower
    st = {}

    def on_item(it):
        want = ref.items[it.k]
        # (shared GPUs: the device and the oracle may name the groups a cycle opens differently, and the feedback carries the names on)
        assert U.same_item(it, want, group_names=not U.has_shared_gpus(it.snap)), f"step {it.k}: the device-built chain leaves the oracle-built one"
        if it.k == 0:
            live["A"] = pkg.KaiCore(abi.copy_config(it.cfg)); st["a"] = live["A"].open_session(it.snap)
            if follower:
                live["F"] = pkg.KaiCore(abi.copy_config(it.cfg)); st["f"] = live["F"].open_session(it.snap)
        else:
            update(st["a"], it)
            assert bytes(live["A"].cfg) == bytes(it.cfg), "the core's configuration follows the rows"
        live["B"] = pkg.KaiCore(abi.copy_config(it.cfg)); st["b"] = live["B"].open_session(it.snap)
        st["opened"] = readback(st["a"])
        assert_readback_equal(st["opened"], readback(st["b"]))
        if follower and it.k:
            update(st["f"], it)
            assert_readback_equal(readback(st["f"]), st["opened"])
        st["it"] = it

    def run(snap, cfg, acts):
        it = st["it"]
        want = ref.items[it.k]
        a, b = st["a"], st["b"]
        raw, ra = cycle(a, acts)
        _, rb = cycle(b, acts)
        assert_cycle_equal(ra, rb)
        res = as_result(raw, ra, st["opened"])
        if U.has_shared_gpus(snap):
            orc = want.res if U.same_snapshot(snap, want.snap) else T.Oracle.run(snap, cfg, acts)  # the oracle on the snapshot with the device's group names
            assert_same_tol(res, orc); _same_groups(snap, res, orc)
            assert res.ops == want.res.ops, "the operations the CPU-built chain was built from"
        else:
            assert_same(res, want.res)
        if it.path is not None:
            assert ra[1][acts.index("allocate")][4] == it.path, f"step {it.k}: the allocate action's path"
        if follower:
            f = st["f"]
            if it.k < len(ref.items) - 1:
                for arr in raw:
                    f.apply_ops(arr)
                assert_readback_equal(readback(f), ra[2])
            else:
                assert_cycle_equal(cycle(f, acts)[1], rb)
        if it.between == "reset":
            a.reset(); b.reset()
            assert_readback_equal(readback(a), readback(b))
            assert_readback_equal(readback(a), st["opened"])
        elif it.between == "query":
            pend = np.nonzero(ra[2]["status"] == U.PENDING)[0]
            if len(pend):
                for x, y in zip(a.best_nodes(pend), b.best_nodes(pend)):
                    assert np.array_equal(x, y), "kai_best_nodes"
                for x, y in zip(a.ordered_nodes(pend, 8), b.ordered_nodes(pend, 8)):
                    assert np.array_equal(x, y), "kai_ordered_nodes"
        live["B"].destroy(); live["B"] = None
        return res

    try:
        chain = U.build(spec, run, on_item)
    finally:
        for c in live.values():
            if c is not None:
                c.destroy()
    assert len(chain.items) == len(ref.items)
    return chain


@pytest.mark.parametrize("seed", U.RANDOM_SEEDS)
def test_gpu_update_chain_random(gpu, seed):  # noqa: F811
    """Six updates over session_case(seed), each the feedback of the cycle before it (placed pods run, evicted ones are Releasing and then Deleted, a few finish, shared-GPU
    groups travel with their pods) merged with a node delta, rows on seeded steps; the follower where kai_ops_apply takes the session."""
    walk(seed, follower=seed % 3 != 2)


@pytest.mark.parametrize("name", [f.__name__ for f in U.SCRIPTED])
def test_gpu_update_chain_scripted(gpu, name):  # noqa: F811
    """One cached quantity of the update walked away, back and away again (the chain's docstring in tests/update_chains.py names it and the path bit of every step)."""
    walk(name)
