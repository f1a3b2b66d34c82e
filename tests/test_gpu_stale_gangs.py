"""kai_stale_gang_eviction on the MI355X.  The expected decision comes from the numpy restatement of the reference's rules (tests/stale_gangs_ref.py), never from the code under
test; the expected state from a twin handle in the same state that takes the call's operations through kai_ops_apply.  The same cases run with emulated lanes in
tests/test_stale_gangs.py."""
import hashlib

import numpy as np
import pytest

import kai_testlib as T
import stale_gangs_ref as R
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
abi = T.abi
S = abi.POD_STATUS
WIDE, ENGINE = abi.APPLY_PATH_WIDE, abi.APPLY_PATH_ENGINE


def read(ssn):
    st, nd = ssn.pod_states()
    return T.Result(pod_status=st, pod_node=nd, nodes=ssn.node_states(), shares=ssn.queue_shares())


def same(got, ref, what=""):
    assert (got.pod_status == ref.pod_status).all() and (got.pod_node == ref.pod_node).all(), f"{what}: pod states, pods {np.nonzero((got.pod_status != ref.pod_status) | (got.pod_node != ref.pod_node))[0][:8].tolist()}"
    for k in ("idle", "releasing", "used"):
        assert got.nodes[k].tobytes() == ref.nodes[k].tobytes(), f"{what}: node {k}"
    for k in ref.shares:
        assert got.shares[k].tobytes() == ref.shares[k].tobytes(), f"{what}: share {k}"


def digest(r):
    h = hashlib.sha256()
    for a in [r.pod_status, r.pod_node] + [r.nodes[k] for k in ("idle", "releasing", "used")] + [r.shares[k] for k in sorted(r.shares)]:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def against_reference(got, ref, what=""):
    ops, since, stale, res = got
    assert np.array_equal(since, ref.since), f"{what}: timestamps, jobs {np.nonzero(since != ref.since)[0][:8].tolist()}"
    assert np.array_equal(stale, ref.expired), f"{what}: Stale, jobs {np.nonzero(stale != ref.expired)[0][:8].tolist()}"
    assert (res.stale_jobs, res.expired_jobs, res.n_ops, res.pad) == (ref.stale_jobs, ref.expired_jobs, len(ref.ops), 0), (what, res.stale_jobs, res.expired_jobs, res.n_ops)
    assert len(ops) == len(ref.ops)
    for f in ("seq", "kind", "pod", "node", "job", "stmt", "pad"):
        assert np.array_equal(ops[f], ref.ops[f]), f"{what}: operations differ in {f} at {np.nonzero(ops[f] != ref.ops[f])[0][:8].tolist()}"


def rows(arr):
    return [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["stmt"])) for o in arr]


@pytest.mark.parametrize("i", range(6))
def test_gpu_reference_cases(gpu, i):
    """actions/stalegangeviction/stalegangeviction_test.go: final pod statuses and nodes (TaskExpectedResults) and the number of evictions (NumberOfCacheEvictions)"""
    line, snap, cfg, since, grace, evictions, meta = R.fixture_cases()[i]
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = ssn.stale_gang_eviction(since, grace)
        assert got[3].n_ops == evictions == len(got[0]), line
        st, nd = ssn.pod_states()
        errs = T.check_expectations(snap, meta, st, nd, None)
        assert not errs, (line, errs)
        against_reference(got, R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, grace), f"case at line {line}")
        ssn.close()


@pytest.mark.parametrize("seed", range(5))
def test_gpu_fuzz_against_the_reference_and_a_twin(gpu, seed):
    """64 nodes, about 20 000 pods in 5 000 jobs (more than 64 workgroups of the pod grid); seed k runs under grace period k mod 3 of {-1, 0, 60 s}"""
    snap, cfg = R.fuzz_snapshot(seed)
    grace = R.GRACES[seed % 3]
    since = R.fuzz_since(snap, seed, grace)
    ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, grace)
    assert (len(ref.ops) == 0) == (grace < 0)
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        before = read(sa)
        dry = sa.stale_gang_eviction(since, grace, dry_run=True)
        against_reference(dry, ref, f"seed {seed} dry run")
        assert digest(read(sa)) == digest(before), "a dry run writes nothing"
        got = sa.stale_gang_eviction(since, grace)
        against_reference(got, ref, f"seed {seed}")
        assert got[3].path == dry[3].path == (ENGINE if len(ref.ops) else abi.APPLY_PATH_NONE), "Pipelined pods among the evicted: the engine walk"
        r = sb.apply_ops(got[0])
        assert r.path == got[3].path
        ra, rb = read(sa), read(sb)
        same(ra, rb, f"seed {seed}: against the twin")
        if len(ref.ops): assert digest(ra) != digest(before)
        pending = np.nonzero(ra.pod_status == S["Pending"])[0][:64]
        assert len(pending) == 64
        na, pa = sa.best_nodes(pending); nb, pb = sb.best_nodes(pending)
        assert np.array_equal(na, nb) and np.array_equal(pa, pb), "best nodes"
        oa, ob = sa.execute("allocate"), sb.execute("allocate")
        assert rows(oa) == rows(ob) and len(oa) > 0, "the following allocate"
        same(read(sa), read(sb), f"seed {seed}: after the following allocate")
        sa.reset()
        same(read(sa), before, "kai_session_reset discards the evictions")
        sa.close(); sb.close()


def test_gpu_apply_paths(gpu):
    """only placed pods in an exact-sum session: the chip-wide path; a Pipelined pod among the evicted: the engine walk"""
    for pipelined, path in ((False, WIDE), (True, ENGINE)):
        snap, cfg = R.fuzz_snapshot(5, n_jobs=600, pipelined=pipelined)
        since = R.fuzz_since(snap, 5, 0)
        ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, 0)
        assert len(ref.ops) > 100 and ((snap.pod_status[ref.ops["pod"]] == S["Pipelined"]).any() == pipelined)
        with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
            sa, sb = a.open_session(snap), b.open_session(snap)
            got = sa.stale_gang_eviction(since, 0)
            against_reference(got, ref, f"pipelined {pipelined}")
            assert got[3].path == path
            assert sb.apply_ops(got[0]).path == path
            same(read(sa), read(sb), f"pipelined {pipelined}: against the twin")
            sa.close(); sb.close()


def test_gpu_capacity_and_refusals(gpu):
    snap, cfg = R.fuzz_snapshot(3, n_jobs=600)
    since = R.fuzz_since(snap, 3, 0)
    ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, 0)
    import ctypes as C
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        before = read(ssn)
        mine = since.copy(); stale = np.full(snap.n_jobs, 9, np.uint8); ops = np.zeros(len(ref.ops), R.OP_DT); n = C.c_int64(-1)
        params = abi.KaiStaleParams(abi.STALE_VERSION, 0, 0)
        rc = core.lib.kai_stale_gang_eviction(core.handle, C.byref(params), mine.ctypes.data_as(C.POINTER(C.c_int64)), stale.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              ops.ctypes.data_as(C.POINTER(abi.KaiOp)), len(ref.ops) - 1, C.byref(n), None)
        assert rc == -4 and n.value == len(ref.ops) and np.array_equal(mine, since) and (stale == 9).all(), "KAI_ERR_CAPACITY: the count needed, the arrays untouched"
        assert digest(read(ssn)) == digest(before)
        core.set_now(0)
        with pytest.raises(T.pkg.core.KaiError) as e:
            ssn.stale_gang_eviction(since, 0)
        assert e.value.code == -1
        core.set_now(R.NOW)
        against_reference(ssn.stale_gang_eviction(since, 0), ref, "after the refusals")
        ssn.close()


def test_gpu_cycle_after_cycle(gpu):
    """the call, its timestamps fed back, the clock moved past the grace period, the call again: the jobs first stamped in call one are evicted in call two and not before"""
    snap, cfg = R.fuzz_snapshot(2, n_jobs=600)
    grace = 60 * R.SEC
    J = snap.n_jobs
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        ref1 = R.decide(snap, snap.pod_status, snap.pod_node, np.zeros(J, np.int64), R.NOW, grace)
        got1 = ssn.stale_gang_eviction(np.zeros(J, np.int64), grace)
        against_reference(got1, ref1, "call one")
        assert ref1.stale_jobs > 10 and len(ref1.ops) == 0 and set(got1[1].tolist()) == {0, R.NOW}, "every stale job is stamped now, nothing is evicted"
        core.set_now(R.NOW + grace - 1)
        got = ssn.stale_gang_eviction(got1[1], grace)
        assert len(got[0]) == 0 and np.array_equal(got[1], got1[1]) and not got[2].any(), "one nanosecond short of the grace period"
        core.set_now(R.NOW + grace)
        st, nd = ssn.pod_states()
        ref2 = R.decide(snap, st, nd, got1[1], R.NOW + grace, grace)
        got2 = ssn.stale_gang_eviction(got1[1], grace)
        against_reference(got2, ref2, "call two")
        assert np.array_equal(got2[2], ref1.stale) and len(got2[0]) > 0, "exactly the jobs stamped in call one"
        # a third cycle: the evicted pods are Releasing — still active-used, so their jobs stay stale and expired, with nothing left to evict
        st, nd = ssn.pod_states()
        ref3 = R.decide(snap, st, nd, got2[1], R.NOW + grace, grace)
        got3 = ssn.stale_gang_eviction(got2[1], grace)
        against_reference(got3, ref3, "call three")
        assert len(got3[0]) == 0 and got3[3].expired_jobs == got2[3].expired_jobs
        ssn.close()
