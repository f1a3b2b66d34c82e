"""kai_session_update on the MI355X: a pod / node delta applied to an open session leaves the handle indistinguishable from one that opened S'
(the snapshot with the delta applied): the same read-backs, bit for bit, and the same operations, states, shares, GPU groups and decision counters from
the cycle that follows, the batch path / sequential engine choice included (kai_action_stats.reserved[4])."""
import copy
import ctypes as C

import numpy as np
import pytest

import kai_testlib as T
from test_gpu_parity import assert_same, assert_same_tol, gpu  # noqa: F401  (fixture)
import test_oracle_golden as _G

pkg = T.pkg
abi = pkg.abi
synth = pkg.synth
CYCLE = ("allocate", "consolidation", "reclaim", "preempt")
PENDING, PIPELINED, BINDING, RUNNING, RELEASING, SUCCEEDED, DELETED = 1, 8, 16, 64, 128, 256, 2048


def readback(ssn):
    st, nd = ssn.pod_states()
    return dict(shares=ssn.queue_shares(), nodes=ssn.node_states(), status=st.copy(), node=nd.copy(), groups=ssn.gpu_groups().copy())


def assert_readback_equal(a, b):
    for k in a["shares"]:
        assert np.array_equal(a["shares"][k], b["shares"][k]), f"shares {k}"
    for k in a["nodes"]:
        assert np.array_equal(a["nodes"][k], b["nodes"][k]), f"nodes {k}"
    for k in ("status", "node", "groups"):
        assert np.array_equal(a[k], b[k]), k


def run_cycle(ssn, actions=CYCLE):
    ops, stats = [], []
    for a in actions:
        arr = ssn.execute(a)
        ops += [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"]), int(o["stmt"])) for o in arr]
        s = ssn.stats()
        stats.append((s.decisions, s.jobs_attempted, s.jobs_committed, s.rollbacks, s.reserved[4] != 0))
    rb = readback(ssn)
    return ops, stats, rb


def assert_cycle_equal(a, b):
    assert a[0] == b[0], "operations"
    assert a[1] == b[1], "decision counters / path"
    assert_readback_equal(a[2], b[2])


def random_delta(snap, rng, frac_groups=True):
    """A legal delta: pending -> running on a node, running -> Releasing / Succeeded / Deleted, Pipelined -> Pending, group changes of fraction pods,
    cordon / NotReady flags and allocatable changes (a node keeps having GPUs or not)."""
    P, N = snap.n_pods, snap.n_nodes
    st, nd = snap.pod_status, snap.pod_node
    flags = snap.pod_flags
    pods, status, node = [], [], []
    portion = snap.arrays.get("pod_gpu_portion")
    for p in rng.permutation(P)[: max(1, P // 6)]:
        s = int(st[p])
        if flags[p] & 0xC:  # CPU fallback / unmodelled: leave them as they are
            continue
        if s == PENDING and N:
            pods.append(p); status.append(RUNNING); node.append(int(rng.integers(0, N)))
        elif s in (RUNNING, BINDING):
            ns = int(rng.choice([RELEASING, SUCCEEDED, DELETED, RUNNING]))
            pods.append(p); status.append(ns); node.append(int(nd[p]) if ns in (RELEASING, RUNNING) else -1)
        elif s == PIPELINED:
            pods.append(p); status.append(PENDING); node.append(-1)
    gpu_group = None
    if frac_groups and portion is not None and (portion > 0).any():
        old = snap.arrays.get("pod_gpu_group", np.full(P, -1, np.int32))
        gpu_group = [int(old[p]) if not (portion[p] > 0 and rng.random() < 0.5) else int(rng.integers(0, 3)) for p in pods]
    nodes = sorted(set(int(x) for x in rng.choice(N, size=min(N, 3), replace=False))) if N else []
    nf = [int(snap.node_flags[n]) ^ (0x1 if rng.random() < 0.5 else 0) for n in nodes]
    alloc = snap.node_allocatable[:, nodes].copy()
    alloc[0] = np.maximum(alloc[0] - 1000 * rng.integers(0, 2, len(nodes)), 1000)  # CPU milli-cores
    gpus = alloc[2]
    alloc[2] = np.where(gpus >= 2, gpus - rng.integers(0, 2, len(nodes)), gpus)  # a GPU node keeps at least one device: its GPU memory rule stays as it was
    if rng.random() < 0.3:
        alloc[0, 0] += 0.5  # a CPU quantity that is no integer: the class guard and the exact-sum guard turn off
    return dict(pods=pods, status=status, node=node, gpu_group=gpu_group, nodes=nodes, node_flags=nf, node_allocatable=alloc)


def session_case(seed):
    snap, cfg, _ = T.broad_case(seed)[0]
    snap = copy.deepcopy(snap)
    if seed % 3 == 2:
        synth.add_fractions(snap, seed, frac=0.3)
    return snap, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_gpu_update_random_sessions(gpu, seed):
    snap, cfg = session_case(seed)
    rng = np.random.default_rng(100 + seed)
    d = random_delta(snap, rng)
    s2 = abi.apply_delta(snap, d["pods"], d["status"], d["node"], d["gpu_group"], d["nodes"], d["node_flags"], d["node_allocatable"])
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a = ca.open_session(snap)
        a.execute("allocate")  # results the update discards
        a.update(d["pods"], d["status"], d["node"], d["gpu_group"], d["nodes"], d["node_flags"], d["node_allocatable"])
        b = cb.open_session(s2)
        assert_readback_equal(readback(a), readback(b))
        ra, rb = run_cycle(a), run_cycle(b)
        assert_cycle_equal(ra, rb)
        a.reset(); b.reset()  # reset returns to S'
        assert_readback_equal(readback(a), readback(b))
    ref = T.Oracle.run(s2, cfg, CYCLE)
    assert [o[:4] for o in ra[0]] == ref.ops
    assert (ra[2]["status"] == ref.pod_status).all() and (ra[2]["node"] == ref.pod_node).all()


def _structure_equal(s1, s2):
    mutable = {"pod_status", "pod_node", "pod_gpu_group", "node_flags", "node_allocatable"}
    if set(s1.arrays) - {"pod_gpu_group"} != set(s2.arrays) - {"pod_gpu_group"} or s1.n_res != s2.n_res:
        return False
    return all(k in mutable or (s1.arrays[k].shape == s2.arrays[k].shape and np.array_equal(s1.arrays[k], s2.arrays[k])) for k in s1.arrays)


def _delta_between(s1, s2):
    pods = np.nonzero((s1.pod_status != s2.pod_status) | (s1.pod_node != s2.pod_node))[0]
    g1 = s1.arrays.get("pod_gpu_group", np.full(s1.n_pods, -1, np.int32)); g2 = s2.arrays.get("pod_gpu_group", np.full(s2.n_pods, -1, np.int32))
    pods = np.union1d(pods, np.nonzero(g1 != g2)[0]).astype(np.int32)
    nodes = np.nonzero((s1.node_flags != s2.node_flags) | (s1.node_allocatable != s2.node_allocatable).any(axis=0))[0].astype(np.int32)
    return dict(pods=pods, status=s2.pod_status[pods], node=s2.pod_node[pods], gpu_group=g2[pods], nodes=nodes, node_flags=s2.node_flags[nodes],
                node_allocatable=s2.node_allocatable[:, nodes])


INTEG = [(n, i, c) for n in _G.INTEG_FILES for i, c in enumerate(T.load_golden(n)["cases"])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,i,case", INTEG, ids=[f"{n}[{i}]" for n, i, _ in INTEG])
def test_gpu_update_integration_rounds(gpu, name, i, case):
    """The integration scenarios with the feedback between rounds applied as kai_session_update on ONE handle (a full open when the structure changed):
    every round equals a fresh open, the expectations hold."""
    from test_engine_hostsim import _same_groups
    state = {"core": None, "ssn": None, "snap": None, "cfg": None, "updates": 0}

    def run_update(snap, cfg, actions):
        if state["core"] is not None and bytes(state["cfg"]) != bytes(cfg):
            state["core"].destroy(); state["core"] = None
        if state["core"] is None:
            state["core"] = pkg.KaiCore(cfg); state["cfg"] = cfg; state["ssn"] = None
        ssn = state["ssn"]
        if ssn is not None and _structure_equal(state["snap"], snap):
            d = _delta_between(state["snap"], snap)
            ssn.update(d["pods"], d["status"], d["node"], d["gpu_group"], d["nodes"], d["node_flags"], d["node_allocatable"])
            state["updates"] += 1
        else:
            ssn = state["core"].open_session(snap)
        state["ssn"], state["snap"] = ssn, snap
        opened = readback(ssn)
        ops, stmts = [], []
        for a in actions:
            arr = ssn.execute(a)
            base = (stmts[-1] + 1) if stmts else 0
            ops += [(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"])) for o in arr]
            stmts += [int(o["stmt"]) + base for o in arr]
        st, nd = ssn.pod_states()
        return T.Result(gpu_groups=ssn.gpu_groups(), ops=ops, stmts=stmts, pod_status=st, pod_node=nd, shares_open=opened["shares"], shares_final=ssn.queue_shares(),
                        nodes=ssn.node_states(), stats=ssn.stats())

    def run_both(snap, cfg, actions):
        from test_gpu_parity import run_gpu
        res = run_update(snap, cfg, actions)
        ref = run_gpu(snap, cfg, actions)
        if "pod_gpu_portion" in snap.arrays:
            assert_same_tol(res, ref); _same_groups(snap, res, ref)
        else:
            assert_same(res, ref)
        return res
    try:
        errs = T.run_integration(case, run_both, rounds_after=1, fractions=True)
    except T.Unsupported as e:
        pytest.skip(str(e))
    finally:
        if state["core"] is not None:
            state["core"].destroy()
    assert not errs, errs[:4]


def _batch_snapshot():
    snap, cfg, _ = synth.config(1, 0.5)
    return snap, cfg


@pytest.mark.gpu
def test_gpu_update_path_flips(gpu):
    """A Releasing pod moves allocate from the batch path to the sequential engine, removing it moves it back: both as fresh opens would."""
    snap, cfg = _batch_snapshot()
    run = np.nonzero(snap.pod_status == RUNNING)[0]
    assert len(run), "the shape needs a running pod"
    p = int(run[0])
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a = ca.open_session(snap)
        ra0 = run_cycle(a, ("allocate",))
        assert ra0[1][0][4], "the shape must take the batch path"
        a.update([p], [RELEASING], [int(snap.pod_node[p])])
        s1 = a.snap
        ra1 = run_cycle(a, ("allocate",))
        rb1 = run_cycle(cb.open_session(s1), ("allocate",))
        assert not ra1[1][0][4], "a Releasing pod: the sequential engine"
        assert_cycle_equal(ra1, rb1)
        a.update([p], [RUNNING], [int(snap.pod_node[p])])
        s2 = a.snap
        ra2 = run_cycle(a, ("allocate",))
        rb2 = run_cycle(cb.open_session(s2), ("allocate",))
        assert ra2[1][0][4], "back on the batch path"
        assert_cycle_equal(ra2, rb2)
        assert ra2[0] == ra0[0]


@pytest.mark.gpu
def test_gpu_update_refusals_leave_session(gpu):
    """Bad arguments, a wrong version, update before open and an open-time refusal: the right status, and the session exactly as it was."""
    snap, cfg = session_case(4)
    P, N = snap.n_pods, snap.n_nodes
    lib = pkg.load_library()
    with pkg.KaiCore(cfg) as core:
        d, _k = pkg.core.delta_struct([0], [PENDING], [-1])
        assert lib.kai_session_update(core.handle, C.byref(d)) == abi_status("STATE")
        ssn = core.open_session(snap)
        before = readback(ssn)
        bad = [([P], [PENDING], [-1], {}), ([0, 0], [PENDING, PENDING], [-1, -1], {}), ([0], [RUNNING], [N], {}),
               ([], [], [], dict(nodes=[N])), ([], [], [], dict(nodes=[0, 0]))]
        for pods, st, nd, kw in bad:
            d, _k = pkg.core.delta_struct(pods, st, nd, **kw)
            assert lib.kai_session_update(core.handle, C.byref(d)) == abi_status("INVALID_ARG"), (pods, kw)
        d, _k = pkg.core.delta_struct([0], [PENDING], [-1], version=7)
        assert lib.kai_session_update(core.handle, C.byref(d)) == abi_status("INVALID_ARG")
        flags = snap.pod_flags.copy(); q = int(np.nonzero(snap.pod_status == PENDING)[0][0])
        assert_readback_equal(readback(ssn), before)
        ops_before = run_cycle(ssn, ("allocate",))[0]
        ssn.reset()
    # an unmodelled pod made active: the open of S' refuses, and so does the update
    s_un = copy.deepcopy(snap); s_un.arrays["pod_flags"] = flags; s_un.arrays["pod_flags"][q] |= 0x8
    with pkg.KaiCore(cfg) as core:
        ssn = core.open_session(s_un)
        before = readback(ssn)
        with pytest.raises(pkg.core.KaiError) as e:
            ssn.update([q], [RUNNING], [0])
        assert e.value.code == abi_status("UNSUPPORTED")
        s2 = abi.apply_delta(s_un, [q], [RUNNING], [0])
        with pkg.KaiCore(cfg) as c2:
            with pytest.raises(pkg.core.KaiError) as e2:
                c2.open_session(s2)
            assert e2.value.code == abi_status("UNSUPPORTED")
        assert_readback_equal(readback(ssn), before)
        assert run_cycle(ssn, ("allocate",))[0] == ops_before


def abi_status(name):
    return {"INVALID_ARG": -1, "UNSUPPORTED": -5, "STATE": -6}[name]


@pytest.mark.gpu
def test_gpu_update_scale_c5(gpu):
    """C5 at 10 %: open, allocate, the next cycle's delta from its operations (placed pods Running, pipelined ones Pending, 1 % of the running pods Succeeded),
    update, allocate — hash-equal to open(S') + allocate."""
    snap, cfg, _ = synth.config(4, 0.1)
    rng = np.random.default_rng(5)
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a = ca.open_session(snap)
        ops = a.execute("allocate")
        d = abi.next_cycle_delta(snap, ops, rng)
        a.update(**d)
        s2 = a.snap
        ha = T.ops_sha256([(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"])) for o in a.execute("allocate")])
        hb = T.ops_sha256([(int(o["kind"]), int(o["pod"]), int(o["node"]), int(o["job"])) for o in cb.open_session(s2).execute("allocate")])
        assert ha == hb



def same_as_open(snap, cfg, d, actions=CYCLE):
    """open(S) + allocate + update(d) on one handle against open(S') on another: equal read-backs and an equal cycle; returns (S', the cycle)."""
    s2 = abi.apply_delta(snap, **d)
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a = ca.open_session(snap)
        a.execute("allocate")
        a.update(**d)
        b = cb.open_session(s2)
        assert_readback_equal(readback(a), readback(b))
        ra, rb = run_cycle(a, actions), run_cycle(b, actions)
        assert_cycle_equal(ra, rb)
    return s2, ra


@pytest.mark.gpu
def test_gpu_update_node_guards_flip(gpu):
    """A node whose CPU allocatable stops being an integer turns the class guard and the exact-sum guard off (allocate leaves the batch path); the next
    delta restores it and the batch path comes back — each as a fresh open of that snapshot decides."""
    snap, cfg = _batch_snapshot()
    R = snap.n_res
    col = snap.node_allocatable[:, [3]].copy()
    bad = col.copy(); bad[0, 0] += 0.5
    with pkg.KaiCore(cfg) as ca, pkg.KaiCore(cfg) as cb:
        a = ca.open_session(snap)
        assert run_cycle(a, ("allocate",))[1][0][4], "the shape must take the batch path"
        a.update([], [], [], nodes=[3], node_allocatable=bad.reshape(R, 1))
        r1 = run_cycle(a, ("allocate",)); b1 = run_cycle(cb.open_session(a.snap), ("allocate",))
        assert not r1[1][0][4]
        assert_cycle_equal(r1, b1)
        a.update([], [], [], nodes=[3], node_allocatable=col.reshape(R, 1))
        r2 = run_cycle(a, ("allocate",)); b2 = run_cycle(cb.open_session(a.snap), ("allocate",))
        assert r2[1][0][4]
        assert_cycle_equal(r2, b2)


@pytest.mark.gpu
def test_gpu_update_class_table_grows(gpu):
    """At open only one request key has pending pods (the class arrays hold one class); the delta makes the pods of every other key pending: the class
    table grows past what the session's arrays held, as open(S') ranks it."""
    snap, cfg = _batch_snapshot()
    req = snap.pod_req
    pend = np.nonzero(snap.pod_status == PENDING)[0]
    keys = {}
    for p in pend:
        keys.setdefault((tuple(req[:, p]), int(snap.pod_class[p])), []).append(int(p))
    assert len(keys) >= 3, "the shape needs several request keys among its pending pods"
    first = next(iter(keys))
    hide = [p for k, ps in keys.items() if k != first for p in ps]
    s0 = abi.apply_delta(snap, hide, [SUCCEEDED] * len(hide), [-1] * len(hide))
    same_as_open(s0, cfg, dict(pods=hide, status=[PENDING] * len(hide), node=[-1] * len(hide)), ("allocate",))


@pytest.mark.gpu
def test_gpu_update_cpu_fallback_refused(gpu):
    """A KAI_POD_CPU_FALLBACK pod made pending: open(S') refuses, so does the update, and the session is as it was."""
    snap, cfg = _batch_snapshot()
    run = np.nonzero(snap.pod_status == RUNNING)[0]
    q = int(run[0])
    s0 = copy.deepcopy(snap); s0.arrays["pod_flags"] = snap.pod_flags.copy(); s0.arrays["pod_flags"][q] |= 0x4
    with pkg.KaiCore(cfg) as core, pkg.KaiCore(cfg) as c2:
        ssn = core.open_session(s0)
        before = readback(ssn); ops0 = run_cycle(ssn, ("allocate",))[0]; ssn.reset()
        with pytest.raises(pkg.core.KaiError) as e:
            ssn.update([q], [PENDING], [-1])
        assert e.value.code == abi_status("UNSUPPORTED")
        with pytest.raises(pkg.core.KaiError) as e2:
            c2.open_session(abi.apply_delta(s0, [q], [PENDING], [-1]))
        assert e2.value.code == abi_status("UNSUPPORTED")
        assert_readback_equal(readback(ssn), before)
        assert run_cycle(ssn, ("allocate",))[0] == ops0


def _shared_snapshot(seed=3):
    snap, cfg, _ = synth.config(1, 0.2)
    snap = copy.deepcopy(snap)
    synth.add_fractions(snap, seed, frac=0.4)
    return snap, cfg


@pytest.mark.gpu
def test_gpu_update_gpu_memory_rule(gpu):
    """Shared GPUs with node_gpu_memory: a CPU-only node that gains devices with the cluster's memory size is applied as open(S') would; with another
    memory size open(S') refuses and so does the update."""
    snap, cfg = _shared_snapshot()
    gm = snap.arrays["node_gpu_memory"]
    cpu_nodes = np.nonzero(snap.node_allocatable[2] == 0)[0]
    if not len(cpu_nodes):  # make one node that holds no pod CPU-only at open
        used = set(int(n) for n in snap.pod_node if n >= 0)
        n0 = next(n for n in range(snap.n_nodes) if n not in used); snap = abi.apply_delta(snap, [], [], [], nodes=[n0], node_allocatable=np.where(np.arange(snap.n_res) == 2, 0.0, snap.node_allocatable[:, n0]).reshape(-1, 1))
    else:
        n0 = int(cpu_nodes[0])
    R = snap.n_res
    col = snap.node_allocatable[:, n0].copy(); col[2] = 4
    same_as_open(snap, cfg, dict(pods=[], status=[], node=[], nodes=[n0], node_allocatable=col.reshape(R, 1)))
    other = copy.deepcopy(snap); other.arrays["node_gpu_memory"] = gm.copy(); other.arrays["node_gpu_memory"][n0] = int(gm.max()) + 100
    with pkg.KaiCore(cfg) as core, pkg.KaiCore(cfg) as c2:
        ssn = core.open_session(other)
        before = readback(ssn)
        with pytest.raises(pkg.core.KaiError) as e:
            ssn.update([], [], [], nodes=[n0], node_allocatable=col.reshape(R, 1))
        assert e.value.code == abi_status("UNSUPPORTED")
        with pytest.raises(pkg.core.KaiError) as e2:
            c2.open_session(abi.apply_delta(other, [], [], [], nodes=[n0], node_allocatable=col.reshape(R, 1)))
        assert e2.value.code == abi_status("UNSUPPORTED")
        assert_readback_equal(readback(ssn), before)


@pytest.mark.gpu
def test_gpu_update_legacy_mig_nodes(gpu):
    """Legacy MIG tasks: moving them between nodes, finishing them and starting them re-marks nodes outside the delta's node list, as open(S') does."""
    snap, cfg, _ = synth.config(1, 0.3)
    snap = copy.deepcopy(snap)
    synth.add_mig(snap, 11, legacy_frac=0.5)
    leg = np.nonzero((snap.pod_flags & 0x10) != 0)[0]
    act = [int(p) for p in leg if snap.pod_status[p] == RUNNING and snap.pod_node[p] >= 0]
    assert act, "the shape needs running legacy MIG tasks"
    N = snap.n_nodes
    pods, st, nd = [], [], []
    for i, p in enumerate(act[:6]):
        pods.append(p)
        if i % 2:
            st.append(SUCCEEDED); nd.append(-1)
        else:
            st.append(RUNNING); nd.append((int(snap.pod_node[p]) + 1) % N)
    same_as_open(snap, cfg, dict(pods=pods, status=st, node=nd))
