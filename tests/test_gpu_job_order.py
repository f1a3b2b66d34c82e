"""kai_job_order on the MI355X.  The expected order comes from the oracle's JobsOrderByQueues (kai_oracle_jobs_order with FilterNonPending | FilterUnready, the depth, n_jobs + 1
pops) on the snapshot whose pod_status / pod_node are the handle's kai_pod_states read-back, never from the code under test; "changes nothing" from the handle's own read-backs
and from a twin handle that never made the call.  The same cases run with emulated lanes in tests/test_job_order.py."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import gpu  # noqa: F401  (fixture)
from test_job_order import TREE, check_positions, oracle_order

pytestmark = pytest.mark.gpu
abi = T.abi
synth = T.pkg.synth
NONE, WIDE, ENGINE = abi.JOB_ORDER_PATH_NONE, abi.JOB_ORDER_PATH_WIDE, abi.JOB_ORDER_PATH_ENGINE


def read(ssn):
    st, nd = ssn.pod_states()
    return T.Result(pod_status=st, pod_node=nd, nodes=ssn.node_states(), shares=ssn.queue_shares())


def digest(ssn):
    r = read(ssn); st = ssn.stats()
    h = hashlib.sha256()
    for a in [r.pod_status, r.pod_node] + [r.nodes[k] for k in ("idle", "releasing", "used")] + [r.shares[k] for k in sorted(r.shares)]:
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(bytes(st))
    return h.hexdigest()


def rows(arr):
    return [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["stmt"])) for o in arr]


def call(ssn, depth=0, engine=False):
    order, pos, qpos, res = ssn.job_order(depth=depth, engine_path=engine)
    return T.Result(order=order, pos=pos.copy(), qpos=qpos.copy(), n=len(order), n_ordered=res.n_ordered, path=res.path, n_leaves=res.n_leaves, pad=res.pad)


def against_oracle(ssn, snap, cfg, depth, want_path=None, what=""):
    """both paths at the session's current state against the oracle and each other; the read-backs and the action statistics as they were"""
    st, nd = ssn.pod_states()
    ref, n_init = oracle_order(abi.apply_delta(snap, np.arange(snap.n_pods), st, nd), cfg, depth)
    before = digest(ssn)
    w, e = call(ssn, depth), call(ssn, depth, engine=True)
    for r, name in ((w, "chip-wide allowed"), (e, "engine path")):
        assert r.n == len(ref) == n_init and r.pad == 0, f"{what} ({name}): {r.n} ordered jobs, the oracle has {len(ref)}"
        assert np.array_equal(r.order, ref), f"{what} ({name}): the order differs from the oracle's at {np.nonzero(r.order != ref)[0][:8].tolist()}"
        check_positions(snap, r, f"{what} ({name})")
    assert e.path == (ENGINE if len(ref) else NONE)
    if want_path is not None: assert w.path == want_path, (what, w.path)
    assert np.array_equal(w.pos, e.pos) and np.array_equal(w.qpos, e.qpos) and w.n_leaves == e.n_leaves
    assert digest(ssn) == before, f"{what}: the call changed a read-back or the action statistics"
    return ref


def shapes():
    out = [("config2", *synth.config(2, 0.05)[:2], WIDE), ("config1", *synth.config(1, 0.3)[:2], None)]
    out += [(f"tree{seed}", synth.make_snapshot(64, 1500, 4200 + seed, **TREE), abi.default_config(), WIDE) for seed in range(3)]
    return out


@pytest.mark.parametrize("i", range(5))
def test_gpu_order_fresh_and_after_an_allocate(gpu, i):
    """both paths, fresh and after one kai_action_execute(allocate), depth 0 and 3: the order and both position arrays are the oracle's, the read-backs are unchanged, and the
    next action commits what a twin handle commits that never made the call"""
    name, snap, cfg, want = shapes()[i]
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        sa, sb = a.open_session(snap), b.open_session(snap)
        fresh = against_oracle(sa, snap, cfg, 0, want, f"{name} fresh")
        against_oracle(sa, snap, cfg, 3, want, f"{name} fresh depth 3")
        oa, ob = sa.execute("allocate"), sb.execute("allocate")
        assert rows(oa) == rows(ob) and len(oa) > 0, "the allocate behind the call against the twin's"
        after = against_oracle(sa, snap, cfg, 0, want, f"{name} after allocate")
        against_oracle(sa, snap, cfg, 3, want, f"{name} after allocate depth 3")
        assert 0 < len(after) < len(fresh)
        if name.startswith("config"):
            assert not np.array_equal(fresh[np.isin(fresh, after)], after), "the survivors' relative order changes with the shares"
        pending = np.nonzero(sa.pod_states()[0] == abi.POD_STATUS["Pending"])[0][:64]
        na, pa = sa.best_nodes(pending); nb, pb = sb.best_nodes(pending)
        assert np.array_equal(na, nb) and np.array_equal(pa, pb), "best nodes"
        for action in ("reclaim", "allocate") if name.startswith("tree") else ("allocate",):  # (a victim action behind the call on the small trees only: every case stays at a few seconds)
            oa, ob = sa.execute(action), sb.execute(action)
            assert rows(oa) == rows(ob), f"the following {action}"
        ra, rb = read(sa), read(sb)
        assert (ra.pod_status == rb.pod_status).all() and (ra.pod_node == rb.pod_node).all()
        for k in rb.shares: assert ra.shares[k].tobytes() == rb.shares[k].tobytes(), k
        sa.close(); sb.close()


def test_gpu_elastic_and_multi_podset_jobs_take_the_engine_path(gpu):
    snap = synth.make_snapshot(64, 1500, 4300, elastic_frac=0.3, multi_podset_frac=0.2, **TREE)
    cfg = abi.default_config()
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        against_oracle(ssn, snap, cfg, 0, None, "elastic fresh")
        assert len(ssn.execute("allocate")) > 0
        ref = against_oracle(ssn, snap, cfg, 0, ENGINE, "elastic after allocate")
        assert len(ref) > 0
        ssn.close()


def test_gpu_fractions_are_not_refused(gpu):
    snap, cfg, _ = synth.config(1, 0.2); synth.add_fractions(snap, 7, frac=0.3)
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        ref = against_oracle(ssn, snap, cfg, 0, None, "fractions")
        assert len(ref) > 100
        ssn.close()


def test_gpu_stream_across_the_scan_tile(gpu):
    """Two leaves of 4 500 one-pod jobs under ONE top-level queue: that queue's merged stream holds 9 000 positions.  k_jo_scan gets 1 024 lanes for a height whose nodes average
    8 192 positions or more, each lane KB_PLAN_SCAN_ELEMS = 4 positions per tile: the stream crosses the tile boundary at position 4 096 and again at 8 192, the running maximum
    carried from tile to tile.  The leaves' own streams cross the leaf kernel's 64-job chunk 70 times."""
    snap = synth.make_snapshot(8, 9000, 78, queue_levels=(1, 2), single_pod_jobs=True, queue_prios=(100, 200), oqws=(1.0, 2.0), usage_max=0.3)
    cfg = abi.default_config()
    with T.pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        ref = against_oracle(ssn, snap, cfg, 0, WIDE, "long stream")
        assert len(ref) == 9000 and np.bincount(snap.job_queue[ref]).max() > 4096
        against_oracle(ssn, snap, cfg, 1000, WIDE, "long stream, depth 1000")
        ssn.close()


def test_gpu_refusals_and_capacity(gpu):
    snap, cfg = synth.config(1, 0.3)[:2]
    J = snap.n_jobs
    I32 = C.POINTER(C.c_int32)

    def raw(core, cap, version=1, flags=0, depth=0):
        order = np.full(J, -7, np.int32); pos = np.full(J, -8, np.int32); qpos = np.full(J, -9, np.int32); n = C.c_int32(-3); r = abi.KaiJobOrderResult(11, 12, 13, 14)
        pm = abi.KaiJobOrderParams(version, flags, depth, 0)
        rc = core.lib.kai_job_order(core.handle, C.byref(pm), order.ctypes.data_as(I32), cap, C.byref(n), pos.ctypes.data_as(I32), qpos.ctypes.data_as(I32), C.byref(r))
        untouched = bool((order == -7).all() and (pos == -8).all() and (qpos == -9).all() and (r.n_ordered, r.path, r.n_leaves, r.pad) == (11, 12, 13, 14))
        return rc, n.value, untouched

    with T.pkg.KaiCore(cfg) as core:
        assert raw(core, J) == (-6, -3, True), "KAI_ERR_STATE without an open session"
        ssn = core.open_session(snap)
        before = digest(ssn)
        assert raw(core, J, version=2) == (-1, -3, True) and raw(core, J, flags=4) == (-1, -3, True) and raw(core, J, depth=-2) == (-1, -3, True)
        full = call(ssn)
        for flags in (0, abi.JOB_ORDER_ENGINE_PATH):
            assert raw(core, full.n - 1, flags=flags) == (-4, full.n, True), "KAI_ERR_CAPACITY: *n_out holds the number needed, the other outputs are untouched"
            assert raw(core, full.n, flags=flags)[:2] == (0, full.n)
        assert digest(ssn) == before
        ssn.close()
        assert raw(core, J) == (-6, -3, True), "KAI_ERR_STATE after kai_session_close"
    with T.pkg.KaiCore(cfg, world=2, rank=0, allgather=lambda send, recv, nbytes: 1) as grp:  # one rank of a two-rank group, formed on this device; it never opens a session
        assert raw(grp, J) == (-5, -3, True), "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
