"""kai_session_update_rows / kai_core_set_now on the MI355X: the cycle's clock, queue rows and job start times applied to an open session, alone or with a
pod / node delta in one call, leave the handle indistinguishable from a fresh handle created with cfg' that opened S' — the same read-backs, bit for bit, and
the same operations, Statement ids, states, shares, groups, decision counters and path from the cycle that follows — also after the victim actions have run
in the session (their replicas and scratch exist), and for arrays the open did not have."""
import copy
import ctypes as C

import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import gpu  # noqa: F401  (fixture)
from test_gpu_session_update import CYCLE, assert_cycle_equal, assert_readback_equal, random_delta, readback, run_cycle, session_case

pkg = T.pkg
abi = pkg.abi
RUNNING = 64
SEC = 1_000_000_000
HOUR = 3600 * SEC


def case(kind, seed):
    snap, cfg, _ = T.broad_case(seed)[0 if kind == "crowded" else -1]
    return copy.deepcopy(snap), abi.copy_config(cfg)


def started_jobs(snap):
    """Jobs that hold a running pod (the ones a snapshot carries a last start time for)."""
    run = snap.pod_job[(snap.pod_status == RUNNING) & (snap.pod_job >= 0)]
    return np.unique(run).astype(np.int32)


def scale_quota(x, f):
    return np.where(x >= 0, x * f, x)  # "unlimited" (-1) stays


def random_rows(snap, cfg, rng):
    """The clock up to +3 h; half the queues' quota rows, usage, priority and min-runtimes; a third of the started jobs' last start in [now - 2 h, now].
    Each optional part is left out now and then (a NULL array)."""
    Q = snap.n_queues
    rows = dict(now_ns=int(cfg.now_ns) + int(rng.integers(0, 3 * 3600 + 1)) * SEC)
    now = rows["now_ns"]
    qs = np.sort(rng.permutation(Q)[: Q // 2]).astype(np.int32)
    if len(qs):
        n = len(qs)
        rows["queues"] = qs
        take = lambda: rng.random() < 0.8
        if take(): rows["queue_deserved"] = scale_quota(snap.queue_deserved[:, qs], rng.choice([0.25, 1.0, 4.0], size=(3, n)))
        if take(): rows["queue_limit"] = scale_quota(snap.queue_limit[:, qs], rng.choice([0.25, 1.0, 4.0], size=(3, n)))
        if take(): rows["queue_oqw"] = rng.choice([1.0, 2.0], size=(3, n))
        if take(): rows["queue_usage"] = rng.random((3, n)) * 0.9
        if take(): rows["queue_priority"] = snap.queue_priority[qs] + rng.choice([0, 500], size=n).astype(np.int32)
        mr = np.array([-1, 0, 600 * SEC, 900 * SEC], np.int64)
        if take(): rows["queue_preempt_min_runtime_ns"] = rng.choice(mr, size=n)
        if take(): rows["queue_reclaim_min_runtime_ns"] = rng.choice(mr, size=n)
    st = started_jobs(snap)
    js = np.sort(rng.permutation(st)[: len(st) // 3]).astype(np.int32)
    if len(js):
        rows["jobs"] = js
        rows["job_last_start_ns"] = now - rng.integers(0, 7200 + 1, size=len(js)).astype(np.int64) * SEC
    return rows


def oracle_ops(snap, cfg):
    return T.Oracle.run(snap, cfg, CYCLE).ops


RANDOM = [("crowded", s) for s in (0, 4, 6, 9, 11, 15, 18, 19)] + [("baseline", s) for s in (0, 2, 4, 7, 14)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", RANDOM, ids=[f"{k}-{s}" for k, s in RANDOM])
def test_gpu_rows_with_delta_random(gpu, kind, seed):
    """Random rows and a random pod / node delta in ONE call, after an allocate whose results the update discards."""
    snap, cfg = case(kind, seed)
    rng = np.random.default_rng(300 + seed)
    d = random_delta(snap, rng)
    rows = random_rows(snap, cfg, rng)
    s2, cfg2 = abi.apply_rows(abi.apply_delta(snap, **d), cfg, **rows)
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg2) as cb:
        a = ca.open_session(snap)
        a.execute("allocate")
        a.update_rows(d, rows)
        assert bytes(ca.cfg) == bytes(cfg2), "Session.update_rows keeps the core's configuration current"
        b = cb.open_session(s2)
        assert_readback_equal(readback(a), readback(b))
        ra, rb = run_cycle(a), run_cycle(b)
        assert_cycle_equal(ra, rb)
        a.reset(); b.reset()  # reset returns to S'
        assert_readback_equal(readback(a), readback(b))
    ref = T.Oracle.run(s2, cfg2, CYCLE)
    assert [o[:4] for o in ra[0]] == ref.ops
    assert (ra[2]["status"] == ref.pod_status).all() and (ra[2]["node"] == ref.pod_node).all()


def perturb(what, snap, cfg):
    Q = snap.n_queues
    if what == "clock":
        return dict(now_ns=int(cfg.now_ns) + 3 * HOUR)
    if what == "last_start":
        js = started_jobs(snap)
        return dict(jobs=js, job_last_start_ns=np.full(len(js), int(cfg.now_ns) - SEC, np.int64))
    if what == "deserved":
        qs = np.arange(max(1, Q // 2), dtype=np.int32)
        return dict(queues=qs, queue_deserved=scale_quota(snap.queue_deserved[:, qs], 0.25))
    if what == "usage":
        qs = np.arange(0, Q, 2, dtype=np.int32)
        return dict(queues=qs, queue_usage=np.full((3, len(qs)), 0.9))
    if what == "priority":
        qs = np.arange(0, Q, 2, dtype=np.int32)
        return dict(queues=qs, queue_priority=snap.queue_priority[qs] + 500)
    raise KeyError(what)


CHANGES = ([("clock", "crowded", s) for s in (6, 9, 15)] + [("last_start", "crowded", s) for s in (6, 15, 18)]
           + [("deserved", "crowded", s) for s in (2, 4, 9)] + [("deserved", "baseline", s) for s in (0, 1)]
           + [("usage", "crowded", s) for s in (4, 11)] + [("usage", "baseline", s) for s in (7, 14)]
           + [("priority", "crowded", s) for s in (2, 7)] + [("priority", "baseline", s) for s in (0, 3)])


@pytest.mark.gpu
@pytest.mark.parametrize("what,kind,seed", CHANGES, ids=[f"{w}-{k}-{s}" for w, k, s in CHANGES])
def test_gpu_rows_change_the_answer(gpu, what, kind, seed):
    """Each kind of row alone, sent with delta = NULL after a whole cycle has run in the session (the victim actions' replicas and scratch exist): the cycle that
    follows is the oracle's on S', cfg' and a fresh open's — and not the one of S, cfg, which the test checks first."""
    snap, cfg = case(kind, seed)
    rows = perturb(what, snap, cfg)
    s2, cfg2 = abi.apply_rows(snap, cfg, **rows)
    ref0, ref = oracle_ops(snap, cfg), T.Oracle.run(s2, cfg2, CYCLE)
    assert ref.ops != ref0, "the rows must change the cycle's operations, or the test shows nothing"
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg2) as cb:
        a = ca.open_session(snap)
        r0 = run_cycle(a)
        assert [o[:4] for o in r0[0]] == ref0
        a.update_rows(None, rows)
        b = cb.open_session(s2)
        assert_readback_equal(readback(a), readback(b))
        ra, rb = run_cycle(a), run_cycle(b)
        assert_cycle_equal(ra, rb)
        assert [o[:4] for o in ra[0]] == ref.ops
        assert (ra[2]["status"] == ref.pod_status).all() and (ra[2]["node"] == ref.pod_node).all()
        a.reset(); b.reset()
        assert_readback_equal(readback(a), readback(b))
        assert_cycle_equal(run_cycle(a), rb)  # a second cycle on S': the replicas carry the rows too
    if what == "clock":  # the same through kai_core_set_now + kai_session_reset
        with pkg.KaiCore(abi.copy_config(cfg)) as cc:
            c = cc.open_session(snap)
            assert_cycle_equal(run_cycle(c), r0)
            cc.set_now(rows["now_ns"])
            assert cc.cfg.now_ns == rows["now_ns"]
            c.reset()
            assert_cycle_equal(run_cycle(c), rb)
            c2 = cc.open_session(snap)  # ... and a later open of the handle runs on the new clock
            assert_cycle_equal(run_cycle(c2), rb)


def open_with_nulls(core, snap):
    """kai_session_open with queue_usage = NULL (a Snapshot always carries the array; zeros are what NULL stands for)."""
    assert not snap.queue_usage.any()
    st = snap.as_struct()
    st.queue_usage = None
    core._check(core.lib.kai_session_open(core.handle, C.byref(st)))
    return pkg.core.Session(core, snap)


@pytest.mark.gpu
def test_gpu_rows_arrays_absent_at_open(gpu):
    """job_last_start_ns, both min-runtime arrays and queue_usage NULL at the open; a cycle runs (replicas laid out without them); rows that name two jobs and two
    queues bring the arrays into being: as a fresh open of S', where they exist.  A second update on top still holds."""
    snap, cfg = case("crowded", 6)
    for k in ("job_last_start_ns", "queue_preempt_min_runtime_ns", "queue_reclaim_min_runtime_ns"):
        assert k in snap.arrays
        del snap.arrays[k]
    snap.arrays["queue_usage"] = np.zeros_like(snap.queue_usage)
    Q = snap.n_queues
    js = started_jobs(snap)
    assert len(js) >= 4 and Q >= 4
    now = int(cfg.now_ns)
    rows1 = dict(queues=[1, Q - 1], queue_usage=np.full((3, 2), 0.5), queue_preempt_min_runtime_ns=[900 * SEC, -1], queue_reclaim_min_runtime_ns=[-1, 600 * SEC],
                 jobs=[int(js[0]), int(js[-1])], job_last_start_ns=[now - SEC, now - 2 * SEC])
    rows2 = dict(now_ns=now + 60 * SEC, queues=[0, 1], queue_usage=np.full((3, 2), 0.1), queue_preempt_min_runtime_ns=[0, 600 * SEC],
                 jobs=[int(js[1]), int(js[-1])], job_last_start_ns=[now - 3 * SEC, 0])
    s1, c1 = abi.apply_rows(snap, cfg, **rows1)
    for k in ("job_last_start_ns", "queue_preempt_min_runtime_ns", "queue_reclaim_min_runtime_ns"):
        assert k in s1.arrays
    s2, c2 = abi.apply_rows(s1, c1, **rows2)
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(c1) as cb, pkg.KaiCore(c2) as cc:
        a = open_with_nulls(ca, snap)
        run_cycle(a)
        a.update_rows(None, rows1)
        b = cb.open_session(s1)
        assert_readback_equal(readback(a), readback(b))
        assert_cycle_equal(run_cycle(a), run_cycle(b))
        a.update_rows(None, rows2)
        c = cc.open_session(s2)
        assert_readback_equal(readback(a), readback(c))
        ra = run_cycle(a)
        assert_cycle_equal(ra, run_cycle(c))
    assert [o[:4] for o in ra[0]] == oracle_ops(s2, c2)


@pytest.mark.gpu
def test_gpu_rows_refusals_leave_session(gpu):
    """A valid delta with bad rows: the status, nothing written (the read-back is unchanged), and the cycle that follows is an untouched twin handle's."""
    snap, cfg = case("crowded", 4)
    Q = snap.n_queues
    d = random_delta(snap, np.random.default_rng(1))
    assert len(d["pods"])
    lib = pkg.load_library()
    with pkg.KaiCore(cfg) as core, pkg.KaiCore(cfg) as twin:
        ssn, ref = core.open_session(snap), twin.open_session(snap)
        before = readback(ssn)
        for kw in (dict(queues=[Q], queue_priority=[1]), dict(jobs=[1, 1], job_last_start_ns=[5, 5]), dict(queues=[0], queue_priority=[1], version=2)):
            ds, _k1 = pkg.core.delta_struct(**d)
            rs, _k2 = pkg.core.rows_struct(**kw)
            assert lib.kai_session_update_rows(core.handle, C.byref(ds), C.byref(rs)) == -1, kw
            assert_readback_equal(readback(ssn), before)
        assert_cycle_equal(run_cycle(ssn), run_cycle(ref))


@pytest.mark.gpu
def test_gpu_rows_null_is_session_update(gpu):
    """kai_session_update_rows(d, NULL) and kai_session_update(d): identical handles."""
    snap, cfg = session_case(7)
    d = random_delta(snap, np.random.default_rng(107))
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a, b = ca.open_session(snap), cb.open_session(snap)
        a.execute("allocate"); b.execute("allocate")
        a.update_rows(d, None)
        b.update(**d)
        assert_readback_equal(readback(a), readback(b))
        assert_cycle_equal(run_cycle(a), run_cycle(b))
        a.reset(); b.reset()
        assert_readback_equal(readback(a), readback(b))
