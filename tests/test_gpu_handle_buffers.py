"""A grown handle answers like a fresh one, on the MI355X.  kai_best_nodes, kai_ops_apply and kai_session_update keep their staging and scratch with the handle
(HandleBuf, kai-scheduler_amd/csrc/kai_handle.hpp) and regrow them when a call needs more: what hangs on a buffer's content (the permutation in kai_best_nodes'
scratch, the zeroed per-pod arrays of kai_ops_apply's) has to be set up again.  One handle makes a small call and then a large one of each kind, a second handle only the
large ones; every answer and the session's state must be equal.  The sizes push kai_best_nodes' and kai_ops_apply's buffers past their 64 KiB floor and the update's staging (which
has none) past what the small call left: tests/test_handle_buffers.py checks with the stand-in runtime's counters that they do (its "C2" cases)."""
import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import gpu  # noqa: F401  (fixture)
from test_ops_apply import ALLOCATE, OP_DT

pytestmark = pytest.mark.gpu
PENDING, RUNNING = T.abi.POD_STATUS["Pending"], T.abi.POD_STATUS["Running"]


def allocate_ops(pods, nodes):
    a = np.zeros(len(pods), OP_DT)
    a["seq"] = a["stmt"] = np.arange(len(pods)); a["kind"] = ALLOCATE; a["pod"] = pods; a["node"] = nodes; a["job"] = -1
    return a


def calls(ssn, snap, small_first):
    """The large call of each kind, behind a small one of the same kind when small_first; the small ones leave the session as it is."""
    P, N = snap.n_pods, snap.n_nodes
    pending = np.nonzero(snap.pod_status == PENDING)[0]
    sets = [np.arange(0, N, 2), np.arange(N // 3, N)]
    out = {}
    if small_first:
        ssn.best_nodes(np.arange(3), sets, [-1, 0, 1])
    out["answers"] = ssn.best_nodes(np.arange(8192) % P, sets, np.arange(8192) % 3 - 1)
    node, _ = ssn.best_nodes(pending)  # every pending pod's best node: the operations below
    out["pending answers"] = node
    if small_first:
        ssn.apply_ops(allocate_ops(pending[:2], np.maximum(node[:2], 0)), check_only=True)
    r = ssn.apply_ops(allocate_ops(pending, np.maximum(node, 0)), check_only=True)
    out["apply_result"] = (r.first_bad, r.path, r.statements)
    if small_first:
        ssn.update(pending[:3], [PENDING] * 3, [-1] * 3)  # (what the snapshot holds already)
    # half the pods in one delta: pending pods, the first on every node that kai_best_nodes named now runs there (it fits: one pod per node), the others stay as they are
    half = pending[:P // 2]
    assert len(half) == P // 2
    _, first = np.unique(node[:len(half)], return_index=True)
    placed = np.array([i for i in first if node[i] >= 0], dtype=np.int64)
    status = np.full(len(half), PENDING, np.int32); where = np.full(len(half), -1, np.int32)
    status[placed] = RUNNING; where[placed] = node[placed]
    ssn.update(half, status, where)
    out["placed"] = len(placed)
    out["pod_states"] = ssn.pod_states()
    out["node_states"] = ssn.node_states()
    out["answers after the update"] = ssn.best_nodes(np.arange(8192) % P, sets, np.arange(8192) % 3 - 1)
    return out


def test_gpu_a_grown_handle_answers_like_a_fresh_one(gpu):  # noqa: F811
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    with T.pkg.KaiCore(cfg) as a, T.pkg.KaiCore(cfg) as b:
        grown, fresh = calls(a.open_session(snap), snap, True), calls(b.open_session(snap), snap, False)
    n_pending = int((snap.pod_status == PENDING).sum())
    assert fresh["apply_result"][0] == -1 and fresh["apply_result"][2] == n_pending and fresh["placed"] >= 1
    assert (fresh["answers"][0] >= 0).any() and (fresh["pod_states"][0] == RUNNING).sum() >= (snap.pod_status == RUNNING).sum() + fresh["placed"]
    assert grown["apply_result"] == fresh["apply_result"] and grown["placed"] == fresh["placed"]
    for k in ("answers", "answers after the update", "pod_states"):
        for x, y in zip(grown[k], fresh[k]):
            assert np.array_equal(x, y), k
    assert np.array_equal(grown["pending answers"], fresh["pending answers"])
    for k in ("idle", "releasing", "used"):
        assert np.array_equal(grown["node_states"][k], fresh["node_states"][k]), k
