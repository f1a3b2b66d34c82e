"""kai_ops_apply on the MI355X.  Operations and expected states come from T.Oracle.run, never from the code under test: the oracle's operations go into a device session
through Session.apply_ops, and pod states, node states and queue shares must be the oracle's, bit for bit — on the chip-wide path, on the engine walk, and for every
action the device runs afterwards.  The same cases at the same sizes run with emulated lanes in tests/test_ops_apply.py."""
import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import crowded, gpu  # noqa: F401  (fixture)
from test_ops_apply import (ALLOCATE, CYCLE, ENGINE, EVICT, PIPELINE, WIDE, WIDE_VICTIM, make_ops, named_twice, per_action, ref_ops, refusal_cases, statement_prefix)

pytestmark = pytest.mark.gpu
abi = T.abi


def read(ssn):
    st, nd = ssn.pod_states()
    return T.Result(pod_status=st, pod_node=nd, nodes=ssn.node_states(), shares=ssn.queue_shares())


def same(got, ref, what="", shares=None):
    assert (got.pod_status == ref.pod_status).all() and (got.pod_node == ref.pod_node).all(), f"{what}: pod states, pods {np.nonzero((got.pod_status != ref.pod_status) | (got.pod_node != ref.pod_node))[0][:8].tolist()}"
    for k in ("idle", "releasing", "used"):
        assert np.array_equal(got.nodes[k], ref.nodes[k]), f"{what}: node {k}"
    shares = shares if shares is not None else (ref.shares if hasattr(ref, "shares") else ref.shares_final)
    for k in shares:
        assert np.array_equal(got.shares[k], shares[k]), f"{what}: share {k}"


def rows(arr):
    return [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"])) for o in arr]


@pytest.fixture(scope="module")
def allocate_case():
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    return snap, cfg, T.Oracle.run(snap, cfg, ("allocate",))


def test_gpu_allocate_batch_on_the_wide_path(gpu, allocate_case):
    snap, cfg, ref = allocate_case
    assert (snap.n_nodes, snap.n_pods, len(ref.ops), len(set(ref.stmts))) == (300, 3277, 649, 196)
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        r = sa.apply_ops(ref_ops(ref))
        assert (r.first_bad, r.path, r.statements) == (-1, WIDE, 196)
        same(read(sa), ref, "the whole action")
        for want in (1, 63, 64, 65, 257):  # prefixes of whole Statements: the chip-wide path on one handle, the engine walk on the other
            n = statement_prefix(ref.stmts, want)
            sa.reset(); sb.reset()
            rw, re_ = sa.apply_ops(ref_ops(ref, 0, n)), sb.apply_ops(ref_ops(ref, 0, n), engine_path=True)
            assert (rw.path, re_.path) == (WIDE, ENGINE) and rw.statements == re_.statements == len(set(ref.stmts[:n]))
            same(read(sa), read(sb), f"prefix of {n}: wide against engine")
            # an allocate action behind either: the same operations and the same end (the oracle has no such run to compare with: its own action, going on behind the
            # prefix, pops the jobs off heaps whose keys were computed before the prefix — a fresh action orders them anew)
            got = [rows(s.execute("allocate")) for s in (sa, sb)]
            assert got[0] == got[1] and len(got[0]) > 0, f"allocate behind a prefix of {n}"
            same(read(sa), read(sb), f"allocate behind a prefix of {n}: wide against engine")
        # at the action's end the oracle can be asked: a second allocate behind the applied first one
        ref2 = T.Oracle.run(snap, cfg, ("allocate", "allocate"))
        sa.reset(); sa.apply_ops(ref_ops(ref))
        assert rows(sa.execute("allocate")) == ref2.ops[len(ref.ops):]
        same(read(sa), ref2, "allocate behind the applied action")
        sa.close(); sb.close()


@pytest.fixture(scope="module")
def crowded_cases():
    return {seed: (crowded(seed),) + per_action(*crowded(seed), CYCLE) for seed in range(12)}


@pytest.mark.parametrize("seed", range(12))
def test_gpu_the_cycle_goes_on(gpu, crowded_cases, seed):
    """the oracle's operations of the first k actions applied, one call per action, the rest of the cycle run by the device: the whole cycle as the oracle ran it"""
    (snap, cfg), ref, cuts = crowded_cases[seed]
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        for k in (1, 2, 3):
            ssn.reset()
            for i in range(k):
                lo, hi = cuts[i], cuts[i + 1]
                r = ssn.apply_ops(ref_ops(ref, lo, hi))
                if hi == lo: assert r.path == abi.APPLY_PATH_NONE
                elif named_twice(ref.ops[lo:hi]): assert r.path == ENGINE, (k, i)
                else: assert r.path in (WIDE, ENGINE)
            ops, stmts = list(ref.ops[:cuts[k]]), list(ref.stmts[:cuts[k]])
            for a in CYCLE[k:]:
                arr = ssn.execute(a)
                base = (stmts[-1] + 1) if stmts else 0  # kai_op.stmt counts from 0 in every action; the oracle numbers a whole cycle
                ops += rows(arr); stmts += [int(o["stmt"]) + base for o in arr]
            assert ops == ref.ops and stmts == ref.stmts, f"k {k}"
            same(read(ssn), ref, f"seed {seed} k {k}")
        ssn.close()


@pytest.mark.parametrize("seed,action,counts", WIDE_VICTIM, ids=[f"crowded{s}-{a}" for s, a, _ in WIDE_VICTIM])
def test_gpu_evictions_and_pipelines_on_the_wide_path(gpu, seed, action, counts):
    snap, cfg = crowded(seed)
    ref = T.Oracle.run(snap, cfg, (action,))
    kinds = [o[0] for o in ref.ops]
    assert (kinds.count(EVICT), kinds.count(PIPELINE)) == counts and not named_twice(ref.ops)
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        assert sa.apply_ops(ref_ops(ref)).path == WIDE and sb.apply_ops(ref_ops(ref), engine_path=True).path == ENGINE
        same(read(sa), ref, "wide"); same(read(sb), read(sa), "engine against wide")
        sa.close(); sb.close()


def test_gpu_follower_handle(gpu):
    """handle A runs the cycle, handle B applies A's operations action by action: equal read-backs and equal best nodes after every action"""
    snap, cfg = crowded(4)
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        for act in CYCLE:
            ops = sa.execute(act)
            r = sb.apply_ops(ops)
            assert r.first_bad == -1
            if len(ops) == 0: assert r.path == abi.APPLY_PATH_NONE
            elif named_twice(rows(ops)): assert r.path == ENGINE, act
            else: assert r.path in (WIDE, ENGINE), act
            ra, rb = read(sa), read(sb)
            same(rb, ra, f"after {act}")
            pending = np.nonzero(ra.pod_status == abi.POD_STATUS["Pending"])[0]
            if len(pending):
                na, pa = sa.best_nodes(pending); nb, pb = sb.best_nodes(pending)
                assert np.array_equal(na, nb) and np.array_equal(pa, pb), f"best nodes after {act}"
        sa.close(); sb.close()


def test_gpu_refusals_write_nothing(gpu):
    snap, cfg = crowded(4)
    ref = T.Oracle.run(snap, cfg, ("allocate",))
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        before = read(sa)
        for name, batch, bad in refusal_cases(snap, ref):
            for kw in ({}, {"engine_path": True}, {"check_only": True}):
                with pytest.raises(T.pkg.core.KaiError) as e:
                    sa.apply_ops(batch, **kw)
                assert e.value.code == -6 and (e.value.result.first_bad, e.value.result.path, e.value.result.statements) == (bad, 0, 0), (name, kw)
                same(read(sa), before, name)
        r = sa.apply_ops(ref_ops(ref), check_only=True)
        assert (r.first_bad, r.statements) == (-1, len(set(ref.stmts)))
        same(read(sa), before, "check only")
        assert rows(sa.execute("reclaim")) == rows(sb.execute("reclaim")), "a following action returns what it returns without the calls"
        same(read(sa), read(sb), "after the following action")
        sa.close(); sb.close()
