"""kai_ordered_nodes on the MI355X: per task the first k nodes of OrderedNodesByTask that pass FittingNode, in the reference's order — against the oracle's lists on
fresh sessions, against the loop of single kai_best_node calls at states only actions reach — and the call changes nothing.

The reference lists are "the best node, asked again with the winners removed from the row", which is the reference's list exactly when the bin-pack pre-order range
cannot move: two anchor nodes in every row (tests/test_ordered_nodes.py: add_anchors, anchors_hold, asserted before anything is asked), or both strategies spread."""
import copy

import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import crowded, gpu  # noqa: F401  (fixture)
from test_gpu_session_update import assert_readback_equal, random_delta, readback
from test_best_nodes import oracle_answers, the_snapshot
from test_gpu_best_nodes import _shared_case, cyc, queries, releasing_snapshot, stats_bytes
from test_ordered_nodes import add_anchors, anchors_hold, as_lists, idle_plus_releasing, oracle_lists, words_of

pytestmark = pytest.mark.gpu
pkg = T.pkg
abi = pkg.abi
synth = pkg.synth
PENDING = 1


def ordered(ssn, q, masks, k):
    node, pipe, count = ssn.ordered_nodes(q["pod"], k, nodesets=masks, nodeset_of=q["nodeset"], pipeline_only=q["flags"] != 0)
    assert node.shape == (len(q), k) and pipe.shape == (len(q), k) and count.shape == (len(q),)
    return as_lists(node, pipe, count)


def single_lists(ssn, q, masks, k):
    """the loop a caller has today, one per DISTINCT query: kai_best_node, the winner removed from the node set, again"""
    N = ssn.snap.n_nodes
    memo = {}
    for x in q:
        key = (int(x["pod"]), int(x["nodeset"]), int(x["flags"]))
        if key in memo: continue
        left = list(range(N)) if key[1] < 0 else np.nonzero(masks[key[1]])[0].tolist()
        lst = []
        while len(lst) < k:
            n, p = ssn.best_node(key[0], pipeline_only=bool(key[2]), nodeset=left)
            if n < 0: break
            lst.append((n, int(p))); left.remove(n)
        memo[key] = lst
    return [memo[(int(x["pod"]), int(x["nodeset"]), int(x["flags"]))] for x in q]


def spread(cfg):
    c = type(cfg).from_buffer_copy(cfg)
    c.gpu_strategy = c.cpu_strategy = abi.SPREAD
    return c


def anchored_masks(N, rng, dens, lo, hi, extra=()):
    masks = [rng.random(N) < d for d in dens] + list(extra)
    for m in masks: m[[lo, hi]] = True
    return masks


def session_ipr(ssn):
    """[R][N] Idle + Releasing as the open session holds it now"""
    ns = ssn.node_states()
    return (ns["idle"] + ns["releasing"]).T


# ---------------------------------------------------------------------------------------------- 1. fresh sessions against the anchored oracle lists
@pytest.mark.parametrize("strat", [abi.BINPACK, abi.SPREAD], ids=["binpack", "spread"])
def test_gpu_ordered_nodes_fresh_session_against_the_oracle_lists(gpu, strat):
    snap = the_snapshot()
    lo, hi = add_anchors(snap)
    N = snap.n_nodes
    rng = np.random.default_rng(31)
    last = np.zeros(N, bool); last[int(np.argmax(snap.arrays["node_name_rank"]))] = True  # only the highest-ranked node (and the anchors)
    masks = anchored_masks(N, rng, (0.0, 0.02, 0.2, 0.7, 1.0), lo, hi, extra=[last])
    assert anchors_hold(snap.arrays["node_allocatable"], idle_plus_releasing(snap), masks, lo, hi)
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    M = 24 * (len(masks) + 1)
    q = queries(np.repeat(rng.choice(pending, size=24, replace=False), len(masks) + 1), cyc(M, len(masks)), (np.arange(M) % 3 == 0).astype(np.uint32))
    cfg = abi.default_config(gpu_strategy=strat, cpu_strategy=strat)
    want = oracle_lists(snap, cfg, masks, q, 8)
    assert all(len(w) == 0 for w, x in zip(want, q) if x["nodeset"] == 0), "the row of the anchors alone answers nothing"
    assert {0, 8} <= {len(w) for w in want} and len({len(w) for w in want}) >= 4, "exhausted and full lists both occur"
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = ordered(ssn, q, masks, 8)
        got1 = ordered(ssn, q, masks, 1)
        node, pipe = ssn.best_nodes(q["pod"], nodesets=masks, nodeset_of=q["nodeset"], pipeline_only=q["flags"] != 0)
        ssn.close()
    assert got == want
    assert got1 == [w[:1] for w in want]
    assert got1 == [([(int(n), int(p))] if n >= 0 else []) for n, p in zip(node, pipe)], "k = 1 is kai_best_nodes, answer for answer"


# ---------------------------------------------------------------------------------------------- 2. Releasing pods: allocatable and pipelined entries in one list
@pytest.mark.parametrize("strat", [abi.BINPACK, abi.SPREAD], ids=["binpack", "spread"])
def test_gpu_ordered_nodes_with_releasing_pods(gpu, strat):
    snap = releasing_snapshot(1008)
    lo, hi = add_anchors(snap)
    N = snap.n_nodes
    assert anchors_hold(snap.arrays["node_allocatable"], idle_plus_releasing(snap), [], lo, hi)
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    q = queries(pending, np.full(len(pending), -1), np.zeros(len(pending), np.uint32))
    cfg = abi.default_config(gpu_strategy=strat, cpu_strategy=strat)
    want = oracle_lists(snap, cfg, [], q, 4)
    assert any(len({p for _, p in w}) == 2 for w in want), "no list holds both allocatable and pipelined entries: pick another seed"
    assert any(len(w) < 4 for w in want) and any(len(w) == 4 for w in want)
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = ordered(ssn, q, [], 4)
        ssn.close()
    assert got == want


# ---------------------------------------------------------------------------------------------- 3. states a fresh open cannot reach; the call changes nothing
@pytest.mark.parametrize("kind", ["c2_after_allocate", "crowded_after_reclaim", "roomy_after_allocate"])
def test_gpu_ordered_nodes_after_an_action_equal_the_single_calls_and_change_nothing(gpu, kind):
    """c2 after allocate is a FULL cluster (measured: no pod of it fits anywhere, every list is empty), so a third state has room left: the_snapshot()'s cluster with 40
    pending pods, after the allocate that placed them — there the lists must be long."""
    rng = np.random.default_rng(33)
    if kind == "c2_after_allocate":
        snap, cfg, _ = synth.config(1, 0.3)
        lo, hi = add_anchors(snap)
        first, nxt = "allocate", "allocate"
    elif kind == "roomy_after_allocate":
        snap = synth.make_snapshot(150, 40, 4242, queue_levels=(2, 2), prefill=0.5, gpu_mix=((8, .5), (4, .3), (0, .2)), cpu_only_frac=0.3, lexi_names=True)
        cfg = abi.default_config()
        lo, hi = add_anchors(snap)
        first, nxt = "allocate", "allocate"
    else:
        snap, cfg = crowded(3)
        cfg = spread(cfg)  # no pre-order: the removal loop is the list (a reclaim may leave Releasing pods on any node, an anchor's too)
        lo = hi = None
        first, nxt = "reclaim", "preempt"
    N = snap.n_nodes
    masks = [rng.random(N) < d for d in (0.1, 0.5, 0.9)]
    if lo is not None:
        for m in masks: m[[lo, hi]] = True
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a, b = ca.open_session(snap), cb.open_session(snap)
        ops_a, ops_b = a.execute(first), b.execute(first)
        assert np.array_equal(ops_a, ops_b) and len(ops_a) > 0
        if lo is not None:
            assert anchors_hold(snap.arrays["node_allocatable"], session_ipr(a), masks, lo, hi), "the anchors hold at the state the action left"
        st, _ = a.pod_states()
        pend, act = np.nonzero(st == PENDING)[0], np.nonzero((st & abi.ACTIVE_USED) != 0)[0]
        pods = np.concatenate([pend, act])  # every pod is asked; the single calls then follow up to 60 tasks that got an answer and 20 that got none
        q_all = queries(pods, cyc(len(pods), len(masks)), (np.arange(len(pods)) % 3 == 0).astype(np.uint32))
        rb0, st0 = readback(a), stats_bytes(a)
        got_all = ordered(a, q_all, masks, 4)
        rb1, st1 = readback(a), stats_bytes(a)
        assert_readback_equal(rb0, rb1)
        assert st0 == st1, "kai_action_stats_get changed"
        lens = np.array([len(g) for g in got_all])
        sel = np.concatenate([np.nonzero(lens > 0)[0][:60], np.nonzero(lens == 0)[0][:20]])
        if kind == "roomy_after_allocate":
            assert (lens[sel] == 4).any() and (lens[sel] > 0).sum() >= 30, "the state the action left answers with full lists"
        assert [got_all[i] for i in sel] == single_lists(a, q_all[sel], masks, 4)
        # the next action: the operations of a twin handle that never made the call
        assert np.array_equal(a.execute(nxt), b.execute(nxt))
        assert_readback_equal(readback(a), readback(b))
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 4. boundaries: every node ties
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_gpu_ordered_nodes_ties_strides_and_words(gpu, N):
    """Uniform empty nodes: every node ties, so a list is the min(k, row size) lowest NAME RANKS of the row in rank order — the tie-break through the insert and through the
    merge across wavefronts, and k above the row's size."""
    snap = synth.make_snapshot(N, 80, 5000 + N, uniform_nodes=True, prefill=0.0, lexi_names=True, cpu_per_gpu=1000.0, mem_per_gpu=1e9)
    rank = snap.arrays["node_name_rank"]
    last_node = np.zeros(N, bool); last_node[N - 1] = True
    last_bits = np.zeros(N, bool); last_bits[31::32] = True; last_bits[N - 1] = True  # the last bit of each word (the last word's last used bit)
    masks = [np.ones(N, bool), last_node, last_bits]
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    pods = pending[: min(32, len(pending))]
    q = queries(np.repeat(pods, 3), np.tile(np.arange(3), len(pods)), np.zeros(3 * len(pods), np.uint32))
    cfg = abi.default_config()
    head = oracle_answers(snap, cfg, words_of(masks, N), q)  # the oracle's k = 1 answer: whether the task fits at all, and is_pipeline (the same on every node)
    by_rank = [np.nonzero(m)[0][np.argsort(rank[m], kind="stable")].tolist() for m in masks]
    assert (head["node"] >= 0).any() and all(h["node"] in (-1, by_rank[x["nodeset"]][0]) for h, x in zip(head, q))
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        for k in (1, 2, 63, 64):
            want = [[(n, int(h["is_pipeline"])) for n in by_rank[x["nodeset"]][:k]] if h["node"] >= 0 else [] for h, x in zip(head, q)]
            assert ordered(ssn, q, masks, k) == want, k
        ssn.close()


# ---------------------------------------------------------------------------------------------- 5. more queries than any grid
def test_gpu_ordered_nodes_more_queries_than_the_grid(gpu):
    snap = synth.make_snapshot(300, 600, 4343, queue_levels=(2, 2), prefill=0.5, gpu_mix=((8, .5), (4, .3), (0, .2)), cpu_only_frac=0.3, lexi_names=True)
    lo, hi = add_anchors(snap)
    N = snap.n_nodes
    rng = np.random.default_rng(34)
    masks = anchored_masks(N, rng, (0.0, 0.02, 0.2, 0.7, 1.0), lo, hi)
    assert anchors_hold(snap.arrays["node_allocatable"], idle_plus_releasing(snap), masks, lo, hi)
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    base = queries(rng.choice(pending, size=300, replace=False), cyc(300, len(masks)), (np.arange(300) % 3 == 0).astype(np.uint32))
    assert len({tuple(x) for x in base.tolist()}) == 300
    q = base[np.arange(5000) % 300]
    cfg = abi.default_config()
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = ordered(ssn, q, masks, 3)
        want = single_lists(ssn, base, masks, 3)
        ssn.close()
    assert got[:300] == want
    assert all(got[i] == got[i % 300] for i in range(5000)), "duplicate queries answer alike"
    assert any(len(g) == 3 for g in got) and any(len(g) == 0 for g in got)


# ---------------------------------------------------------------------------------------------- 6. shared GPUs, GPU-memory requests, MIG
@pytest.mark.parametrize("seed", [4, 7])
@pytest.mark.parametrize("kind", ["fraction", "gpu_memory", "mig"])
def test_gpu_ordered_nodes_shared_gpus_memory_requests_and_mig(gpu, kind, seed):
    snap, cfg = _shared_case(kind, seed)
    cfg = spread(cfg)  # no pre-order: the removal loop is the list
    N = snap.n_nodes
    rng = np.random.default_rng(35 + seed)
    masks = [rng.random(N) < 0.5, np.ones(N, bool)]
    ok = np.nonzero((snap.arrays["pod_flags"] & 0xC) == 0)[0]
    q = queries(ok, cyc(len(ok), len(masks)), (np.arange(len(ok)) % 3 == 0).astype(np.uint32))
    want = oracle_lists(snap, cfg, masks, q, 3)
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = ordered(ssn, q, masks, 3)
        assert got == want, "fresh session against the oracle's lists"
        assert any(len(g) > 1 for g in got)
        ssn.execute("allocate")
        assert ordered(ssn, q, masks, 3) == single_lists(ssn, q, masks, 3), "after allocate against the single calls"
        ssn.close()


# ---------------------------------------------------------------------------------------------- 7. a second, larger call on the same handle; a call after kai_session_update
def test_gpu_ordered_nodes_second_larger_call_and_after_an_update(gpu):
    snap, cfg, _ = T.broad_case(3)[0]
    snap = copy.deepcopy(snap)
    cfg = spread(cfg)  # (the delta below moves pods and flags freely: no anchors to keep)
    N = snap.n_nodes
    rng = np.random.default_rng(36)
    ok = np.nonzero((snap.arrays["pod_flags"] & 0xC) == 0)[0]
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        m1 = [rng.random(N) < 0.5]
        q1 = queries(ok[:8], cyc(8, 1), np.zeros(8, np.uint32))
        want1 = oracle_lists(snap, cfg, m1, q1, 2)
        assert ordered(ssn, q1, m1, 2) == want1
        # more queries, more rows and a larger k than the first call sized the scratch for
        m2 = [rng.random(N) < d for d in np.linspace(0.05, 0.95, 40)]
        M2 = 6000
        q2 = queries(ok[np.arange(M2) % len(ok)], cyc(M2, len(m2)), (np.arange(M2) % 3 == 0).astype(np.uint32))
        got2 = ordered(ssn, q2, m2, 16)
        uniq = min(400, M2)
        assert got2[:uniq] == oracle_lists(snap, cfg, m2, q2[:uniq], 16)
        memo = {}
        for x, g in zip(q2.tolist(), got2):
            assert memo.setdefault(tuple(x), g) == g, "duplicate queries answer alike"
        assert ordered(ssn, q1, m1, 2) == want1, "a smaller call on the grown scratch"
        node, pipe = ssn.best_nodes(q2["pod"], nodesets=m2, nodeset_of=q2["nodeset"], pipeline_only=q2["flags"] != 0)
        assert [g[:1] for g in got2] == [([(int(n), int(p))] if n >= 0 else []) for n, p in zip(node, pipe)], "kai_best_nodes on the scratch the two share"
        assert ordered(ssn, q1, m1, 2) == want1
        # after kai_session_update the handle equals one that opened S': against the oracle on S'
        d = random_delta(snap, rng)
        ssn.update(d["pods"], d["status"], d["node"], d["gpu_group"], d["nodes"], d["node_flags"], d["node_allocatable"])
        s2 = ssn.snap
        ok2 = np.nonzero((s2.arrays["pod_flags"] & 0xC) == 0)[0]
        q3 = queries(ok2[np.arange(300) % len(ok2)], cyc(300, len(m2)), (np.arange(300) % 3 == 0).astype(np.uint32))
        assert ordered(ssn, q3, m2, 5) == oracle_lists(s2, cfg, m2, q3, 5)
        ssn.close()
