"""Spread placement on the GPU (`gpu_strategy = SPREAD`, plugins/nodeplacement/spread.go:16-36) on the set-based fill kernels.

When every class asks for a whole number of devices, k_bucket_build's proof holds and every node with a free device divides by ONE device count, the reference orders
the fitting nodes of a class by (free devices descending, name rank ascending): the best node of any class is the first node of the highest non-empty level, a task moves it
from level g to g - q.  The spread instantiations of k_fill_levels (up to 8 levels) and k_fill_counts (9 - 16 levels, KAI_FILL_TWO_WORKERS) run that on the sets (DESIGN.md
5.2e); everything else under spread — several divisors, a class with a static bitmap, the one-wave and unbatched switches — stays on the general k_fill.

CPU part: the kernels' bodies on the emulator of kai_simt.hpp inside tests/host_sim.  Every case compares operations, pod states, node accounting, shares and the four counters
with the oracle and, where the sets ran, with the general kernel (KAI_FILL_GENERAL=1) on the same snapshot.  tests/test_gpu_fill_spread.py runs the same cases on the MI355X
through the C ABI: the cases below take the backend as an argument.  (No case sets KAI_HOSTSIM_NATIVE_FILL: the scalar shadow of tests/host_sim is bin-pack only.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
from test_engine_hostsim import HostSim, assert_same

abi = T.abi
synth = T.pkg.synth
GIB = synth.GIB


def stats_tuple(s):
    return (s.decisions, s.jobs_attempted, s.jobs_committed, s.rollbacks)


class Sim:
    """the emulator: stats.reserved[6] = actions on the sets, reserved[7] = on k_fill_counts (low word) / k_fill_levels (high word)"""
    run = staticmethod(lambda snap, cfg: HostSim.run(snap, cfg))
    same = staticmethod(assert_same)
    on_buckets = staticmethod(lambda res: int(res.stats.reserved[6]) == 1)
    on_counts = staticmethod(lambda res: (int(res.stats.reserved[7]) & 0xffffffff) == 1)
    on_levels = staticmethod(lambda res: (int(res.stats.reserved[7]) >> 32) == 1)
    rounds = staticmethod(lambda res: int(res.stats.reserved[5]))


def spread_cfg(**kw):
    return abi.default_config(gpu_strategy=abi.SPREAD, k_value=0.5, **kw)


def check(B, snap, cfg, monkeypatch, sets=True):
    """the oracle, the backend, and — where the sets ran — the general kernel on the same snapshot; returns the backend's result"""
    ref = T.Oracle.run(snap, cfg)
    res = B.run(snap, cfg)
    B.same(res, ref)
    assert stats_tuple(res.stats) == stats_tuple(ref.stats)
    assert res.stats.reserved[4] >= 1, "the allocate action did not take the batch path"
    if sets is not None:
        assert B.on_buckets(res) == sets, "the fill ran on the sets" if not sets else "the fill did not run on the sets"
    if B.on_buckets(res):
        assert B.on_counts(res), "a spread session on the sets runs a counting machine"
        monkeypatch.setenv("KAI_FILL_GENERAL", "1")
        gen = B.run(snap, cfg)
        monkeypatch.delenv("KAI_FILL_GENERAL")
        assert not B.on_buckets(gen) and gen.stats.reserved[4] >= 1
        B.same(gen, ref); assert stats_tuple(gen.stats) == stats_tuple(ref.stats)
    return res


# ---------------------------------------------------------------------------------------------- random one-divisor clusters
SEEDS = list(range(24))
DECLINED = (7, 10, 19, 22)  # a resource other than the devices may bind first on some node: k_bucket_build's proof fails, under either strategy


def seed_devices(seed):
    return (8, 16, 4)[seed % 3]


def seed_snapshot(seed):
    """nodes of ONE device count (8, 16 or 4), prefill 0 .. 0.9, gangs of up to 100 tasks, requests of 1 / 2 / 4 / 8 or 1 / 3 / 5 devices cut to the node's size"""
    rng = np.random.default_rng(8800 + seed)
    g = seed_devices(seed)
    sizes, probs = ((1, 2, 3, 24), (.3, .2, .2, .3)) if seed % 2 else ((1, 4, 8, 16, 64, 100), (.1, .2, .3, .2, .1, .1))
    per_pod = tuple(x for x in ((1, 2, 4, 8) if seed % 4 else (1, 3, 5)) if x <= g)
    return synth.make_snapshot(int(rng.integers(2, 300)), int(rng.integers(20, 2500)), 8800 + seed, queue_levels=[(1,), (2, 2), (3, 4), (2, 2, 2)][seed % 4],
                               prefill=(0.0, 0.3, 0.6, 0.9)[seed % 4], gpu_mix=((g, 1.0),), gpus_per_pod=per_pod, gang_sizes=sizes, gang_p=probs,
                               mem_per_gpu=8 * GIB, cpu_per_gpu=2000.0, lexi_names=bool(seed % 5 == 0))


def case_random(B, seed, monkeypatch):
    snap = seed_snapshot(seed)
    res = check(B, snap, spread_cfg(), monkeypatch, sets=None)
    pack = B.run(snap, abi.default_config(k_value=0.5))
    assert B.on_buckets(res) == B.on_buckets(pack), "the proof is strategy-independent: spread and bin-pack qualify alike"
    assert B.on_buckets(res) == (seed not in DECLINED)
    if not B.on_buckets(res):
        return
    g = seed_devices(seed)
    assert B.on_counts(res) and B.on_levels(res) == (g in (4, 8))  # (16-device nodes: more levels than k_fill_levels has wavefronts for)
    if g in (4, 8):  # the spread form of k_fill_counts on the same snapshot
        monkeypatch.setenv("KAI_FILL_TWO_WORKERS", "1")
        two = B.run(snap, spread_cfg())
        monkeypatch.delenv("KAI_FILL_TWO_WORKERS")
        assert B.on_counts(two) and not B.on_levels(two)
        B.same(two, res); assert stats_tuple(two.stats) == stats_tuple(res.stats)


@pytest.mark.parametrize("seed", SEEDS)
def test_spread_random_one_divisor_clusters(seed, monkeypatch):
    case_random(Sim, seed, monkeypatch)


def test_spread_seeds_mostly_run_on_the_sets():
    """at least 20 of the 24 clusters pass the proof (a generator that skips more hides a failure)"""
    assert len(SEEDS) - len(DECLINED) >= 20
    for seed in DECLINED:
        assert not Sim.on_buckets(HostSim.run(seed_snapshot(seed), abi.default_config(k_value=0.5))), seed


# ---------------------------------------------------------------------------------------------- hand-made cases
def tiny(free, gangs, devices=8, lexi=False, label=None):
    """nodes of `devices` devices with free[i] of them free (a running filler pod holds the rest), one queue, the pending gangs in the order given: gangs[j] = the devices
    every pod of gang j asks for.  label: node -> node_gpu_count other than its devices."""
    N = len(free); R = 4
    alloc = np.zeros((R, N)); alloc[abi.RES_CPU] = 128000.0; alloc[abi.RES_MEM] = 512 * GIB; alloc[abi.RES_GPU] = devices; alloc[abi.RES_PODS] = 110
    used = [devices - f for f in free]; run_nodes = [i for i in range(N) if used[i] > 0]
    sizes = [len(g) for g in gangs] + [1] * len(run_nodes)
    J = len(sizes); P = sum(sizes); npend = sum(len(g) for g in gangs)
    dev = np.array([float(x) for g in gangs for x in g] + [float(used[i]) for i in run_nodes])
    req = np.zeros((R, P)); req[abi.RES_GPU] = dev; req[abi.RES_CPU] = 2000.0 * dev; req[abi.RES_MEM] = 8 * GIB * dev; req[abi.RES_PODS] = 1.0
    names = [(f"node-{i}" if lexi else f"node-{i:06d}") for i in range(N)]
    qt = synth._queue_tree([1], np.random.default_rng(1), float(devices * N))
    snap = abi.Snapshot(n_res=R); a = snap.arrays
    a["node_allocatable"] = alloc; a["node_flags"] = np.zeros(N, np.uint32)
    cnt = np.full(N, devices, np.int32)
    for i, v in (label or {}).items(): cnt[i] = v
    a["node_gpu_count"] = cnt
    a["node_name_rank"] = abi.rank_strings(names) if lexi else np.arange(N, dtype=np.uint32)
    a["pod_req"] = req; a["pod_job"] = np.repeat(np.arange(J, dtype=np.int32), sizes); a["pod_podset"] = np.repeat(np.arange(J, dtype=np.int32), sizes)
    st = np.full(P, abi.POD_STATUS["Pending"], np.int32); st[npend:] = abi.POD_STATUS["Running"]
    nd = np.full(P, -1, np.int32); nd[npend:] = run_nodes
    a["pod_status"] = st; a["pod_node"] = nd; a["pod_uid_rank"] = np.arange(P, dtype=np.uint32)
    a["podset_job"] = np.arange(J, dtype=np.int32); a["podset_min_available"] = np.array(sizes, np.int32); a["podset_name_rank"] = np.zeros(J, np.uint32)
    a["job_queue"] = np.full(J, qt["leaves"][0], np.int32); a["job_priority"] = np.full(J, 50, np.int32); a["job_preemptible"] = np.ones(J, np.int32)
    a["job_created_ns"] = (np.arange(J, dtype=np.int64) + 1) * 60_000_000_000; a["job_uid_rank"] = np.arange(J, dtype=np.uint32); a["job_signature"] = np.full(J, 50, np.int64)
    a["job_first_pod"] = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32); a["job_n_pods"] = np.array(sizes, np.int32)
    a["job_first_podset"] = np.arange(J, dtype=np.int32); a["job_n_podsets"] = np.ones(J, np.int32)
    a["queue_parent"] = qt["parent"]; a["queue_priority"] = qt["prio"]; a["queue_created_ns"] = qt["created"]; a["queue_uid_rank"] = np.arange(len(qt["parent"]), dtype=np.uint32)
    a["queue_deserved"] = qt["deserved"]; a["queue_limit"] = qt["limit"]; a["queue_oqw"] = qt["oqw"]; a["queue_usage"] = qt["usage"]
    snap.node_names = names; snap.queue_names = qt["names"]
    snap.finalize()
    return snap


def placed(res, lo, hi):
    """nodes of the pending pods lo .. hi - 1 (-1: not placed)"""
    return [int(x) for x in res.pod_node[lo:hi]]


def case_step_draws_from_the_level_the_step_before_filled(B, monkeypatch):
    """8, 8 and 5 free: the gang's first two tasks take the two nodes of level 8 down to level 6, the third finds level 6 on top — node 0 again"""
    res = check(B, tiny([8, 8, 5], [[2, 2, 2]]), spread_cfg(), monkeypatch)
    assert placed(res, 0, 3) == [0, 1, 0]
    assert B.on_levels(res)


def case_rollback_then_next_job(B, monkeypatch):
    """two nodes with 4 free hold four tasks of 2 devices: a gang of five books 5 decisions and is rolled back; the 4-device pod behind it lands on node 0"""
    res = check(B, tiny([4, 4], [[2] * 5, [4]], devices=4), spread_cfg(), monkeypatch)
    assert placed(res, 0, 5) == [-1] * 5 and placed(res, 5, 6) == [0]
    assert stats_tuple(res.stats) == (6, 2, 1, 2)


def case_lexicographic_names(B, monkeypatch):
    """ties go to the lower NAME: node-10 sorts before node-2"""
    res = check(B, tiny([8] * 12, [[1], [1], [1]], lexi=True), spread_cfg(), monkeypatch)
    assert placed(res, 0, 3) == [0, 1, 10]


def case_stretch_of_one_task_gangs(B, monkeypatch):
    """more than 64 one-task gangs in a row: a full stretch of the counting machine, every gang one command of one node"""
    res = check(B, tiny([8, 7, 8, 3, 8, 8, 6, 8, 1, 8], [[1 + (j % 2)] for j in range(90)]), spread_cfg(), monkeypatch)
    assert all(n >= 0 for n in placed(res, 0, 39)) and res.stats.jobs_committed == 46  # (65 free devices: the cluster fills up inside the second stretch)


def case_short_gang_third_step(B, monkeypatch):
    """a gang of 3 tasks on levels that hold one node each: three steps — the run holds two commands in lanes, the third sends the gang the long way"""
    res = check(B, tiny([8, 7, 6, 2], [[1], [1, 1, 1], [1, 1, 1, 1, 1], [2]]), spread_cfg(), monkeypatch)
    # [1] -> node 0 (8 -> 7); then levels: 7 {0, 1}, 6 {2}: the gang of three takes 0, 1 (-> 6) and then the first node of level 6
    assert placed(res, 0, 4) == [0, 0, 1, 0]


def case_two_classes_in_one_gang(B, monkeypatch):
    """a gang whose pods ask for 1 and for 4 devices: task by task on the counts"""
    res = check(B, tiny([8, 8, 5, 3], [[1, 4, 1, 4], [4, 1], [1, 4, 4, 4, 4, 4, 4]]), spread_cfg(), monkeypatch)
    assert all(n >= 0 for n in placed(res, 0, 6)) and len(set(placed(res, 0, 4))) >= 2  # (where each task lands: the comparison with the oracle in check())


def case_second_level_summary(B, monkeypatch):
    """about 4 200 nodes: the sets' second summary level holds more than one word"""
    rng = np.random.default_rng(8899)
    free = [int(x) for x in rng.integers(0, 5, size=4200)]
    gangs = [[int(rng.choice((1, 2, 4)))] * int(rng.choice((1, 1, 2, 30))) for _ in range(400)]
    res = check(B, tiny(free, gangs, devices=4), spread_cfg(), monkeypatch)
    assert B.on_levels(res)


HAND = [case_step_draws_from_the_level_the_step_before_filled, case_rollback_then_next_job, case_lexicographic_names, case_stretch_of_one_task_gangs,
        case_short_gang_third_step, case_two_classes_in_one_gang, case_second_level_summary]


@pytest.mark.parametrize("case", HAND, ids=[c.__name__[5:] for c in HAND])
def test_spread_hand_made(case, monkeypatch):
    case(Sim, monkeypatch)


@pytest.mark.parametrize("case", HAND[:6], ids=[c.__name__[5:] for c in HAND[:6]])
def test_spread_hand_made_on_the_two_worker_kernel(case, monkeypatch):
    """the same cases on the spread form of k_fill_counts"""
    monkeypatch.setenv("KAI_FILL_TWO_WORKERS", "1")
    case(type("SimTwo", (Sim,), {"on_levels": staticmethod(lambda res: True)}), monkeypatch)


# ---------------------------------------------------------------------------------------------- declines: the general kernel, still on the batch path
def case_decline_two_divisors(B, monkeypatch):
    """8- and 4-device nodes: nodes of one ratio free / count with different counts neither fit alike nor move alike"""
    snap = synth.make_snapshot(120, 900, 8850, queue_levels=(2, 2), prefill=0.3, gpu_mix=((8, .6), (4, .4)), mem_per_gpu=8 * GIB, cpu_per_gpu=2000.0)
    assert B.on_buckets(B.run(snap, abi.default_config(k_value=0.5))), "the cluster qualifies under bin-pack"
    check(B, snap, spread_cfg(), monkeypatch, sets=False)


def case_decline_one_label_changed(B, monkeypatch):
    """one node's nvidia.com/gpu.count label says 16 on a cluster of 8-device nodes"""
    free = [8, 8, 5, 8, 2, 8]
    gangs = [[2, 2, 2], [1], [4, 4], [1] * 6]
    check(B, tiny(free, gangs), spread_cfg(), monkeypatch, sets=True)
    check(B, tiny(free, gangs, label={3: 16}), spread_cfg(), monkeypatch, sets=False)


def case_decline_one_wave_and_unbatched(B, monkeypatch):
    """k_fill_buckets is bin-pack only: the switches that select it leave a spread session on the general kernel"""
    snap = seed_snapshot(1)
    for var in ("KAI_FILL_ONE_WAVE", "KAI_FILL_UNBATCHED"):
        monkeypatch.setenv(var, "1")
        check(B, snap, spread_cfg(), monkeypatch, sets=False)
        monkeypatch.delenv(var)


def case_decline_static_bitmap(B, monkeypatch):
    """pod classes x node classes: a class looks its nodes up through a bitmap of its own — bin-pack runs k_fill_buckets, spread the general kernel"""
    rng = np.random.default_rng(8860)
    snap = synth.make_snapshot(80, 600, 8860, queue_levels=(2, 3), prefill=0.3, mem_per_gpu=8 * GIB, cpu_per_gpu=2000.0)
    a = snap.arrays
    a["node_class"] = rng.integers(0, 3, size=snap.n_nodes).astype(np.int32)
    a["pod_class"] = np.repeat(rng.integers(0, 2, size=snap.n_jobs), a["job_n_pods"]).astype(np.int32)
    a["class_fit"] = np.array([[1, 1, 0], [1, 0, 1]], np.uint8)
    snap.finalize()
    pack = B.run(snap, abi.default_config(k_value=0.5))
    assert B.on_buckets(pack) and not B.on_counts(pack)
    check(B, snap, spread_cfg(), monkeypatch, sets=False)


DECLINES = [case_decline_two_divisors, case_decline_one_label_changed, case_decline_one_wave_and_unbatched, case_decline_static_bitmap]


@pytest.mark.parametrize("case", DECLINES, ids=[c.__name__[13:] for c in DECLINES])
def test_spread_declines(case, monkeypatch):
    case(Sim, monkeypatch)


# ---------------------------------------------------------------------------------------------- wave schedules (the emulator only)
@pytest.mark.parametrize("two_workers", [0, 1])
@pytest.mark.parametrize("order", [1, 2])
def test_spread_under_other_wave_schedules(order, two_workers):
    """the waves of the workgroup in reverse order and with random passes sat out (kai_simt.hpp KW_EMU_ORDER, read once per process): the results stay the oracle's"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import kai_testlib as T\nimport test_fill_spread as S\n"
            "for seed in (0, 2, 3, 4, 8):\n"
            "    snap = S.seed_snapshot(seed); cfg = S.spread_cfg()\n"
            "    ref = T.Oracle.run(snap, cfg); res = S.HostSim.run(snap, cfg)\n"
            "    assert S.Sim.on_counts(res) and S.Sim.on_levels(res) == (not %d and seed %% 3 != 1), seed\n"
            "    S.assert_same(res, ref); assert S.stats_tuple(res.stats) == S.stats_tuple(ref.stats), seed\n") % (os.path.join(T.ROOT, "tests"), two_workers)
    env = dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="7")
    if two_workers: env["KAI_FILL_TWO_WORKERS"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- the round loop
def case_round_loop(B, seed, monkeypatch):
    """the loop on the device against the loop on the host, with short first plans (many rounds, mispredictions): equal operations, counters and rounds"""
    snap = seed_snapshot(seed); cfg = spread_cfg()
    monkeypatch.setenv("KAI_BATCH_H0", "8")
    dev = check(B, snap, cfg, monkeypatch)
    monkeypatch.setenv("KAI_BATCH_HOST_LOOP", "1")
    host = B.run(snap, cfg)
    assert B.on_buckets(host) and host.stats.reserved[4] >= 1
    B.same(host, dev); assert stats_tuple(host.stats) == stats_tuple(dev.stats)
    assert B.rounds(host) == B.rounds(dev), "the two loops took different numbers of rounds"


@pytest.mark.parametrize("seed", [2, 9])
def test_spread_round_loop_on_the_device_against_the_host(seed, monkeypatch):
    case_round_loop(Sim, seed, monkeypatch)


# ---------------------------------------------------------------------------------------------- the BASELINE shapes, scaled
SCALED = [(4, 0.03), (1, 0.2)]  # config 5 and config 2


def case_scaled_config(B, idx, scale, monkeypatch):
    snap, cfg, _ = synth.config(idx, scale)
    cfg.gpu_strategy = abi.SPREAD
    res = check(B, snap, cfg, monkeypatch)
    assert B.on_levels(res)


@pytest.mark.parametrize("idx,scale", SCALED)
def test_spread_scaled_baseline_configs(idx, scale, monkeypatch):
    case_scaled_config(Sim, idx, scale, monkeypatch)
