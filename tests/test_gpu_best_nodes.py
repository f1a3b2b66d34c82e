"""kai_best_nodes on the MI355X: out[i] is exactly what kai_best_node answers for queries[i] at the same session state — against the oracle on fresh sessions, against the
loop of single calls at states only actions reach — and the call changes nothing: read-backs, statistics and the next action are those of a handle that never made it."""
import copy
import ctypes as C

import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import crowded, gpu  # noqa: F401  (fixture)
from test_gpu_session_update import assert_readback_equal, random_delta, readback
from test_best_nodes import oracle_answers, the_snapshot

pytestmark = pytest.mark.gpu
pkg = T.pkg
abi = pkg.abi
synth = pkg.synth
PENDING, RUNNING, RELEASING = 1, 64, 128
Q_DT = np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("pad", "<i4")])


def words_of(masks, N):
    w = np.zeros((len(masks), max((N + 31) // 32, 1)), np.uint32)
    for s, m in enumerate(masks):
        idx = np.nonzero(m)[0]
        np.bitwise_or.at(w[s], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return w


def queries(pods, rows, flags):
    q = np.zeros(len(pods), Q_DT)
    q["pod"], q["nodeset"], q["flags"] = pods, rows, flags
    return q


def batched(ssn, q, masks):
    node, pipe = ssn.best_nodes(q["pod"], nodesets=masks, nodeset_of=q["nodeset"], pipeline_only=q["flags"] != 0)
    return list(zip(node.tolist(), pipe.astype(int).tolist()))


def singles(ssn, q, masks):
    """the loop of kai_best_node calls, one per DISTINCT query"""
    memo = {}
    for x in q:
        k = (int(x["pod"]), int(x["nodeset"]), int(x["flags"]))
        if k not in memo:
            n, p = ssn.best_node(k[0], pipeline_only=bool(k[2]), nodeset=None if k[1] < 0 else np.nonzero(masks[k[1]])[0].tolist())
            memo[k] = (n, int(p))
    return [memo[(int(x["pod"]), int(x["nodeset"]), int(x["flags"]))] for x in q]


def as_list(ans):
    return list(zip(ans["node"].tolist(), ans["is_pipeline"].tolist()))


def stats_bytes(ssn):
    return bytes(ssn.stats())


def density_masks(N, rng, dens=(0.0, 0.02, 0.2, 0.7)):
    return [rng.random(N) < d for d in dens] + [np.ones(N, bool)]


def cyc(n, k, lo=-1):
    return (np.arange(n) % (k - lo)) + lo


# ---------------------------------------------------------------------------------------------- 1. fresh sessions against the oracle
@pytest.mark.parametrize("strat", [abi.BINPACK, abi.SPREAD], ids=["binpack", "spread"])
def test_gpu_best_nodes_fresh_session_against_the_oracle(gpu, strat):
    snap = the_snapshot()
    N = snap.n_nodes
    rng = np.random.default_rng(21)
    last = np.zeros(N, bool); last[int(np.argmax(snap.arrays["node_name_rank"]))] = True  # only the highest-ranked node
    masks = density_masks(N, rng) + [last]
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    q = queries(rng.choice(pending, size=96), cyc(96, len(masks)), (np.arange(96) % 3 == 0).astype(np.uint32))
    cfg = abi.default_config(gpu_strategy=strat, cpu_strategy=strat)
    want = as_list(oracle_answers(snap, cfg, words_of(masks, N), q))
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = batched(ssn, q, masks)
        ssn.close()
    assert got == want
    assert all(w == (-1, 0) for w, x in zip(want, q) if x["nodeset"] == 0), "the empty row answers -1"
    assert any(w[0] >= 0 for w in want)


RELEASING_SEED = 1007


def releasing_snapshot(seed=RELEASING_SEED):
    """a crowded 12-node cluster in which a fifth of the Running pods are Releasing before the open"""
    snap = synth.make_crowded_snapshot(12, seed)
    rng = np.random.default_rng(seed)
    run = np.nonzero(snap.arrays["pod_status"] == RUNNING)[0]
    snap.arrays["pod_status"][rng.choice(run, size=len(run) // 5, replace=False)] = RELEASING
    return snap


@pytest.mark.parametrize("strat", [abi.BINPACK, abi.SPREAD], ids=["binpack", "spread"])
def test_gpu_best_nodes_with_releasing_pods_against_the_oracle(gpu, strat):
    snap = releasing_snapshot()
    N = snap.n_nodes
    rng = np.random.default_rng(22)
    masks = density_masks(N, rng, dens=(0.0, 0.2, 0.5))
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    M = 96
    q = queries(pending[np.arange(M) % len(pending)], cyc(M, len(masks)), (np.arange(M) % 3 == 0).astype(np.uint32))
    cfg = abi.default_config(gpu_strategy=strat, cpu_strategy=strat)
    want = as_list(oracle_answers(snap, cfg, words_of(masks, N), q))
    # the oracle alone: a placement on releasing resources nobody asked for, a task nothing fits, a task that fits
    assert any(w[0] >= 0 and w[1] == 1 and x["flags"] == 0 for w, x in zip(want, q)), "no pipelined answer without PIPELINE_ONLY: pick another seed"
    assert any(w[0] == -1 and x["nodeset"] != 0 for w, x in zip(want, q)) and any(w[0] >= 0 for w in want)
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = batched(ssn, q, masks)
        ssn.close()
    assert got == want


# ---------------------------------------------------------------------------------------------- 2. states a fresh open cannot reach
def _after_action_case(kind):
    if kind == "c2_after_allocate":
        snap, cfg, _ = synth.config(1, 0.3)
        return snap, cfg, "allocate", "allocate"
    snap, cfg = crowded(3)
    return snap, cfg, "reclaim", "preempt"


@pytest.mark.parametrize("kind", ["c2_after_allocate", "crowded_after_reclaim"])
def test_gpu_best_nodes_after_an_action_equal_the_single_calls_and_change_nothing(gpu, kind):
    snap, cfg, first, nxt = _after_action_case(kind)
    N = snap.n_nodes
    rng = np.random.default_rng(23)
    masks = [rng.random(N) < d for d in (0.1, 0.5, 0.9)]
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a, b = ca.open_session(snap), cb.open_session(snap)
        ops_a, ops_b = a.execute(first), b.execute(first)
        assert np.array_equal(ops_a, ops_b)
        st, _ = a.pod_states()
        pend, act = np.nonzero(st == PENDING)[0], np.nonzero((st & abi.ACTIVE_USED) != 0)[0]
        pods = np.concatenate([pend, rng.choice(act, size=min(50, len(act)), replace=False)])
        q = queries(pods, cyc(len(pods), len(masks)), (np.arange(len(pods)) % 3 == 0).astype(np.uint32))
        rb0, st0 = readback(a), stats_bytes(a)
        got = batched(a, q, masks)
        rb1, st1 = readback(a), stats_bytes(a)
        assert_readback_equal(rb0, rb1)
        assert st0 == st1, "kai_action_stats_get changed"
        assert got == singles(a, q, masks)
        # the next action: the operations of a twin handle that never made the call
        assert np.array_equal(a.execute(nxt), b.execute(nxt))
        assert_readback_equal(readback(a), readback(b))
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 3. boundaries of the strides and of the bitmap words
@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025])
def test_gpu_best_nodes_stride_and_word_boundaries(gpu, N):
    """Every node ties (uniform empty nodes), so the answer is the lowest NAME RANK of the row — which is not its lowest index."""
    snap = synth.make_snapshot(N, 80, 5000 + N, uniform_nodes=True, prefill=0.0, lexi_names=True, cpu_per_gpu=1000.0, mem_per_gpu=1e9)
    rank = snap.arrays["node_name_rank"]
    assert N < 11 or (np.argsort(rank) != np.arange(N)).any()
    last_node = np.zeros(N, bool); last_node[N - 1] = True
    last_bits = np.zeros(N, bool); last_bits[31::32] = True; last_bits[N - 1] = True  # the last bit of each word (the last word's last used bit)
    masks = [np.ones(N, bool), last_node, last_bits]
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    pods = pending[: min(64, len(pending))]
    q = queries(np.repeat(pods, 3), np.tile(np.arange(3), len(pods)), np.zeros(3 * len(pods), np.uint32))
    cfg = abi.default_config()
    want = as_list(oracle_answers(snap, cfg, words_of(masks, N), q))
    lowest = [int(np.nonzero(m)[0][np.argmin(rank[m])]) for m in masks]
    assert any(w[0] >= 0 for w in want) and all(w[0] in (-1, lowest[x["nodeset"]]) for w, x in zip(want, q)), "the oracle's own answers: the lowest name rank of the row"
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = batched(ssn, q, masks)
        ssn.close()
    assert got == want


# ---------------------------------------------------------------------------------------------- 4. more queries than any grid
def test_gpu_best_nodes_more_queries_than_the_grid(gpu):
    snap = synth.make_snapshot(300, 600, 4343, queue_levels=(2, 2), prefill=0.5, gpu_mix=((8, .5), (4, .3), (0, .2)), cpu_only_frac=0.3, lexi_names=True)
    N = snap.n_nodes
    rng = np.random.default_rng(24)
    masks = density_masks(N, rng)
    pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0]
    base = queries(rng.choice(pending, size=300, replace=False), cyc(300, len(masks)), (np.arange(300) % 3 == 0).astype(np.uint32))
    assert len({tuple(x) for x in base.tolist()}) == 300
    q = base[np.arange(5000) % 300]
    cfg = abi.default_config()
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = batched(ssn, q, masks)
        want = singles(ssn, base, masks)
        ssn.close()
    assert got[:300] == want
    assert all(got[i] == got[i % 300] for i in range(5000)), "duplicate queries answer alike"
    assert any(g[0] >= 0 for g in got) and any(g[0] < 0 for g in got)


# ---------------------------------------------------------------------------------------------- 5. shared GPUs, GPU-memory requests, MIG
def _shared_case(kind, seed):
    kw = dict(fill=0.3 + 0.5 * (seed % 5) / 4, n_pending_jobs=6 + seed % 13, elastic_frac=0.2, hog_frac=0.5, queue_levels=((2, 2), (3,), (2, 2, 2))[seed % 3],
              cpu_only_frac=0.3 if seed % 4 == 0 else 0.0)
    if kind == "fraction":  # the generator of test_gpu_fraction_fuzz
        snap = synth.make_crowded_snapshot(2 + seed % 9, 9300 + seed, **kw)
        synth.add_fractions(snap, seed, frac=0.6, portions=(0.25, 0.5, 0.75))
        cfg = abi.default_config(gpu_strategy=(abi.BINPACK, abi.SPREAD)[seed % 2], cpu_strategy=(abi.BINPACK, abi.SPREAD)[(seed // 2) % 2], k_value=(0.0, 0.5, 1.0)[seed % 3],
                                 max_consolidation_preemptees=(-1, 16, 2)[seed % 3])
        if seed % 3 == 0: cfg.plugins = (cfg.plugins & ~abi.PLUGINS["gpupack"]) | abi.PLUGINS["gpuspread"]
        if seed % 7 == 0: cfg.plugins &= ~abi.PLUGINS["gpusharingorder"]
    elif kind == "gpu_memory":  # test_gpu_gpu_memory_fuzz
        snap = synth.make_crowded_snapshot(2 + seed % 9, 9900 + seed, **kw)
        synth.add_fractions(snap, seed, frac=0.7, memory_requests=(0.5, 1.0)[seed % 2], gpu_memory=(100, 200, 16300)[seed % 3], portions=(0.25, 0.5, 0.75))
        cfg = abi.default_config(gpu_strategy=(abi.BINPACK, abi.SPREAD)[seed % 2], k_value=(0.0, 0.5, 1.0)[seed % 3])
        cfg.min_node_gpu_memory = (100, 200, 16300)[seed % 3] if seed % 5 else 100
        if seed % 3 == 0: cfg.plugins = (cfg.plugins & ~abi.PLUGINS["gpupack"]) | abi.PLUGINS["gpuspread"]
    else:  # test_gpu_mig_fuzz
        snap = synth.make_crowded_snapshot(3 + seed % 9, 4400 + seed, **kw)
        synth.add_mig(snap, seed, node_frac=(0.3, 0.6, 1.0)[seed % 3], pod_frac=(0.5, 0.9)[seed % 2], legacy_frac=(0.0, 0.05, 0.2)[seed % 3])
        cfg = abi.default_config(gpu_strategy=(abi.BINPACK, abi.SPREAD)[seed % 2], k_value=(0.0, 0.5, 1.0)[seed % 3], max_consolidation_preemptees=(-1, 16, 2)[seed % 3])
    return snap, cfg


@pytest.mark.parametrize("seed", [4, 7])
@pytest.mark.parametrize("kind", ["fraction", "gpu_memory", "mig"])
def test_gpu_best_nodes_shared_gpus_memory_requests_and_mig(gpu, kind, seed):
    snap, cfg = _shared_case(kind, seed)
    N = snap.n_nodes
    rng = np.random.default_rng(25 + seed)
    masks = [rng.random(N) < 0.5, np.ones(N, bool)]
    ok = np.nonzero((snap.arrays["pod_flags"] & 0xC) == 0)[0]
    q = queries(ok, cyc(len(ok), len(masks)), (np.arange(len(ok)) % 3 == 0).astype(np.uint32))
    want = as_list(oracle_answers(snap, cfg, words_of(masks, N), q))
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        got = batched(ssn, q, masks)
        assert got == want, "fresh session against the oracle"
        assert any(g[0] >= 0 for g in got)
        ssn.execute("allocate")
        assert batched(ssn, q, masks) == singles(ssn, q, masks), "after allocate against the single calls"
        ssn.close()


# ---------------------------------------------------------------------------------------------- 6. a second, larger call on the same handle; a call after kai_session_update
def test_gpu_best_nodes_second_larger_call_and_after_an_update(gpu):
    snap, cfg, _ = T.broad_case(3)[0]
    snap = copy.deepcopy(snap)
    N, P = snap.n_nodes, snap.n_pods
    rng = np.random.default_rng(26)
    ok = np.nonzero((snap.arrays["pod_flags"] & 0xC) == 0)[0]
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(snap)
        m1 = [rng.random(N) < 0.5]
        q1 = queries(ok[:8], cyc(8, 1), np.zeros(8, np.uint32))
        assert batched(ssn, q1, m1) == as_list(oracle_answers(snap, cfg, words_of(m1, N), q1))
        # more queries and more rows than the first call sized the scratch for
        m2 = [rng.random(N) < d for d in np.linspace(0.05, 0.95, 40)]
        M2 = 6000
        q2 = queries(ok[np.arange(M2) % len(ok)], cyc(M2, len(m2)), (np.arange(M2) % 3 == 0).astype(np.uint32))
        got2 = batched(ssn, q2, m2)
        uniq = min(M2, len(ok) * (len(m2) + 1) * 3)
        assert got2[:uniq] == singles(ssn, q2[:uniq], m2)
        assert batched(ssn, q1, m1) == as_list(oracle_answers(snap, cfg, words_of(m1, N), q1)), "a smaller call on the grown scratch"
        # after kai_session_update the handle equals one that opened S': against the oracle on S'
        d = random_delta(snap, rng)
        ssn.update(d["pods"], d["status"], d["node"], d["gpu_group"], d["nodes"], d["node_flags"], d["node_allocatable"])
        s2 = ssn.snap
        ok2 = np.nonzero((s2.arrays["pod_flags"] & 0xC) == 0)[0]
        q3 = queries(ok2[np.arange(400) % len(ok2)], cyc(400, len(m2)), (np.arange(400) % 3 == 0).astype(np.uint32))
        got3 = batched(ssn, q3, m2)
        assert got3 == as_list(oracle_answers(s2, core.cfg, words_of(m2, N), q3))
        assert got3 == singles(ssn, q3, m2)
        ssn.close()
