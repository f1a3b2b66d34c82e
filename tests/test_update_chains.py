"""The chains of tests/update_chains.py, built with the oracle as the runner: are they worth running?  These are conditions on the INPUTS of
tests/test_gpu_update_chains.py — the library is not called here (under the CPU suite's stand-in runtime the delta kernels do nothing, so the update cannot be
held to anything without the device).  Every condition is asserted: a chain that stops meeting one shows nothing on the MI355X either.

Seeds of session_case that had to be left out of the random chains (SKIPPED_SEEDS): 8, which would have been a third shared-GPU seed, and 15 — their clusters
fill up within three cycles, and fewer than four of the seven cycles commit an operation; test_skipped_seeds_are_skipped_for_their_reason keeps the list honest.
The other seeds of range(20) meet the conditions; the eight taken are those whose cycles go on committing longest (4, 9, 11 and 18 commit in exactly four), with
three shared-GPU seeds among them."""
import numpy as np
import pytest

import kai_testlib as T
import update_chains as U

abi = T.pkg.abi
SKIPPED_SEEDS = (8, 15)  # fewer than four cycles that commit an operation


def committing(chain):
    return sum(1 for it in chain.items if len(it.res.ops) > 0)


@pytest.mark.parametrize("seed", U.RANDOM_SEEDS)
def test_random_chain_is_worth_running(seed):
    ch = U.oracle_chain(seed)
    assert len(ch.items) == U.RandomChain.K + 1 == 7
    rows, plain = 0, 0
    for it in ch.items[1:]:
        d = it.delta
        assert len(d["pods"]) + len(d["nodes"]) > 0, f"step {it.k}: an empty delta"
        assert len(set(d["pods"])) == len(d["pods"]) and len(set(d["nodes"])) == len(d["nodes"]), f"step {it.k}: listed twice"
        rows += it.rows is not None; plain += it.rows is None
    assert rows >= 1 and plain >= 1, "both entry points in every chain"
    assert {it.between for it in ch.items} == {None, "reset", "query"}
    assert committing(ch) >= 4, [len(it.res.ops) for it in ch.items]
    for it in ch.items:
        it.snap.as_struct()
    # the feedback: what a cycle evicted is Releasing in the next snapshot and Deleted in the one after
    for a, b in zip(ch.items, ch.items[1:]):
        was = a.snap.pod_status == U.RELEASING
        assert (b.snap.pod_status[was] == U.DELETED).all() and (b.snap.pod_node[was] == -1).all()
        evicted = np.asarray(a.res.pod_status) == U.RELEASING
        assert (b.snap.pod_status[evicted & ~was] == U.RELEASING).all()
        assert not (b.snap.pod_status & (U.PIPELINED | U.ALLOCATED | U.BINDING)).any(), "a status only a cycle leaves"


def test_random_chains_cover_the_paths_evictions_and_new_groups():
    chains = [U.oracle_chain(s) for s in U.RANDOM_SEEDS]
    assert len(U.RANDOM_SEEDS) == 8 and sum(1 for s in U.RANDOM_SEEDS if s % 3 == 2) >= 2
    paths = {U.predict_path(it.snap, it.cfg) for ch in chains for it in ch.items}
    assert paths == {U.BATCH, U.ENGINE}
    assert sum(1 for ch in chains if any(o[0] == 2 for it in ch.items for o in it.res.ops)) >= 2, "evictions in two seeds at least"
    # shared GPUs: group ids at and above KAI_NEW_GROUP enter the snapshots with the feedback and leave them again
    for ch, seed in zip(chains, U.RANDOM_SEEDS):
        if seed % 3 != 2:
            continue
        assert all(U.has_shared_gpus(it.snap) for it in ch.items)
    fr = [ch for ch, seed in zip(chains, U.RANDOM_SEEDS) if seed % 3 == 2]
    counts = [[sum(U.new_groups(it.snap).values()) for it in ch.items] for ch in fr]
    assert any(any(b > a for a, b in zip(c, c[1:])) for c in counts) and any(any(b < a for a, b in zip(c, c[1:])) for c in counts), counts


@pytest.mark.parametrize("seed", SKIPPED_SEEDS)
def test_skipped_seeds_are_skipped_for_their_reason(seed):
    assert committing(U.build(U.RandomChain(seed), T.Oracle.run)) < 4


def _chain(fn):
    ch = U.oracle_chain(fn.__name__)
    for it in ch.items:
        it.snap.as_struct()
    rows = [it.rows is not None for it in ch.items[1:]]
    assert any(rows) and not all(rows), "both entry points in every chain"
    return ch


def test_scripted_chains_name_what_the_rule_says():
    """Where a scripted chain names the path bit and the snapshot rule (predict_path) says ENGINE, the chain says ENGINE; where the chain says BATCH the rule does.
    (guards_cpu_zero's ENGINE steps are the ones the rule cannot see: a class guard that fails on integers.)"""
    for fn in U.SCRIPTED:
        ch = _chain(fn)
        for it in ch.items:
            if it.path is None:
                assert fn is U.rows_appear_late
                continue
            rule = U.predict_path(it.snap, it.cfg)
            if it.path == U.BATCH or fn is not U.guards_cpu_zero:
                assert rule == it.path, (ch.name, it.k)


def test_guards_cpu_fraction_states():
    ch = _chain(U.guards_cpu_fraction)
    cpu = lambda s: int((s.node_allocatable[abi.RES_CPU] != np.floor(s.node_allocatable[abi.RES_CPU])).sum())
    assert [cpu(it.snap) for it in ch.items] == [it.state for it in ch.items] == [0, 2, 1, 0]
    assert [it.path for it in ch.items] == [U.BATCH, U.ENGINE, U.ENGINE, U.BATCH]


def test_guards_cpu_zero_states():
    ch = _chain(U.guards_cpu_zero)
    zero = lambda s: int((s.node_allocatable[abi.RES_CPU] == 0).sum())
    assert [zero(it.snap) for it in ch.items] == [it.state for it in ch.items] == [0, 2, 1, 0]
    assert [it.path for it in ch.items] == [U.BATCH, U.ENGINE, U.ENGINE, U.BATCH]
    for it in ch.items:  # every quantity stays an integer (the exact-sum guard passes throughout) and CPU-only pods are pending
        assert (it.snap.node_allocatable == np.floor(it.snap.node_allocatable)).all()
        assert any(not (k[0][abi.RES_GPU] > 0) for k in U.pending_keys(it.snap))
    used = set(int(n) for n in ch.items[0].snap.pod_node if n >= 0)
    assert not used & set(ch.items[1].delta["nodes"]), "the nodes that lose their CPUs hold no pod"


def test_guards_exact_sums_states():
    ch = _chain(U.guards_exact_sums)
    assert [U.exact_sums_state(it.snap) for it in ch.items] == [it.state for it in ch.items] == [(0, False), (1, False), (0, True), (0, False), (1, False), (0, False)]
    assert [it.path for it in ch.items] == [U.BATCH, U.ENGINE, U.ENGINE, U.BATCH, U.ENGINE, U.BATCH]
    # the edge itself: at step 2 the sum is exactly 2 ** 52 units of one byte, at step 3 one less
    total = lambda s: sum(int(v) for v in s.node_allocatable[abi.RES_MEM])
    assert total(ch.items[2].snap) == 1 << 52 and total(ch.items[3].snap) == (1 << 52) - 1
    for it in ch.items:  # CPU and GPU rows untouched: the class guard passes throughout
        assert np.array_equal(it.snap.node_allocatable[[0, 2, 3]], ch.items[0].snap.node_allocatable[[0, 2, 3]])


def test_releasing_by_count_states():
    ch = _chain(U.releasing_by_count)
    assert [int((it.snap.pod_status == U.RELEASING).sum()) for it in ch.items] == [it.state for it in ch.items] == [0, 2, 1, 0]
    assert [it.path for it in ch.items] == [U.BATCH, U.ENGINE, U.ENGINE, U.BATCH]
    assert ch.items[3].res.ops == ch.items[0].res.ops and ch.items[1].res.ops != ch.items[0].res.ops
    assert U.same_snapshot(ch.items[3].snap, ch.items[0].snap)


def test_class_table_states():
    ch = _chain(U.class_table)
    n = [len(U.pending_keys(it.snap)) for it in ch.items]
    assert n == [it.state for it in ch.items] and n[0] == n[2] == n[3] == 1 and n[1] == n[4] >= 3
    assert U.pending_keys(ch.items[2].snap) == U.pending_keys(ch.items[0].snap) != U.pending_keys(ch.items[3].snap)
    assert all(len(it.res.ops) > 0 for it in ch.items)


def test_delta_sizes_states():
    ch = _chain(U.delta_sizes)
    sizes = [(len(it.delta["pods"]), len(it.delta.get("nodes", []))) for it in ch.items[1:]]
    assert sizes == list(U.DELTA_SIZES) == [it.state for it in ch.items[1:]]
    assert {p for p, _ in sizes} >= {0, 1, 3, 255, 256, 257, 1025} and {n for _, n in sizes} == {0, 1, 3}
    assert any(p % 256 and n for p, n in sizes) and any(p and p % 256 == 0 and n for p, n in sizes), "the node section inside a workgroup and on a boundary"
    for a, b in zip(ch.items, ch.items[1:]):
        d = b.delta
        pods = np.asarray(d["pods"], np.int64)
        changed = (a.snap.pod_status[pods] != np.asarray(d["status"])) | (a.snap.pod_node[pods] != np.asarray(d["node"]))
        if len(pods):
            assert changed[-1], f"step {b.k}: the last pod entry changes nothing"
        if len(pods) > 3:
            assert not changed.all() and changed.sum() >= min(len(pods) // 4, 64), f"step {b.k}: entries the snapshot holds already, and real ones"
        for i, nn in enumerate(d.get("nodes", [])):
            assert a.snap.node_flags[nn] != d["node_flags"][i] and a.snap.node_allocatable[0, nn] != d["node_allocatable"][0][i], f"step {b.k}: node entry {i} changes nothing"
        assert not (b.snap.pod_status & (U.RELEASING | U.PIPELINED)).any()
    assert all(it.path == U.BATCH for it in ch.items)


def test_rows_appear_late_states():
    ch = _chain(U.rows_appear_late)
    held = [tuple(k for k in U.LATE_ARRAYS if k in it.snap.arrays) for it in ch.items]
    assert held == [it.state for it in ch.items] == [(), (), U.LATE_ARRAYS[:2], U.LATE_ARRAYS[:2], U.LATE_ARRAYS]
    assert [(it.delta is not None, it.rows is not None) for it in ch.items[1:]] == [(True, False), (False, True), (True, False), (True, True)]
    assert ch.actions == U.CYCLE
    assert not set(ch.items[2].rows["queues"]) & set(ch.items[4].rows["queues"]) and not set(ch.items[2].rows["jobs"]) & set(ch.items[4].rows["jobs"])


def test_legacy_mig_states():
    ch = _chain(U.legacy_mig)
    n = ch.info["node"]
    assert [U.legacy_on(it.snap, n) for it in ch.items] == [it.state for it in ch.items] == [2, 1, 0, 1, 2]
    listed = [n in (it.delta.get("nodes") or []) for it in ch.items[1:]]
    assert listed == [True, False, False, False]
    assert ch.items[0].snap.node_flags[n] & abi.NODE_NOT_READY and not ch.items[1].snap.node_flags[n] & abi.NODE_NOT_READY
    assert [bool(it.delta.get("nodes")) for it in ch.items[1:]] == [True, True, False, True], "n's own entry behind the delta's nodes, and alone"
    on_n = [sum(1 for o in it.res.ops if o[0] == 0 and o[2] == n) for it in ch.items]
    assert on_n[2] > 0 and on_n[0] == on_n[1] == on_n[3] == on_n[4] == 0, "the legacy bit decides whether the cycle places on n"


def test_shared_gpus_states():
    ch = _chain(U.shared_gpus)
    x, A, B = ch.info["x"], ch.info["A"], ch.info["B"]
    assert [(int(it.snap.pod_node[x]) == B, U.new_groups(it.snap)) for it in ch.items] == [it.state for it in ch.items]
    assert [int(it.snap.pod_node[x]) for it in ch.items] == [A, B, B, A, B, A, A, A]
    G = U.NEW_GROUP
    assert [U.new_groups(it.snap) for it in ch.items] == [{}, {G: 1}, {G: 1}, {}, {G + 5: 2}, {G + 5: 1}, {}, {G: 1}]
    s0 = ch.items[0].snap
    assert s0.pod_uid_rank[x] == 0 and not np.array_equal(np.argsort(s0.pod_uid_rank), np.arange(s0.n_pods)), "UID order is not index order, x is first in it"
    for it in ch.items:  # every cycle opens groups of its own: the first id it hands out (next_group0) shows in the group read-back
        want = max(U.new_groups(it.snap), default=G - 1) + 1
        got = np.asarray(it.res.gpu_groups)
        assert (got >= want).any() and set(int(g) for g in got[(got >= G) & (got < want)]) <= set(U.new_groups(it.snap))
