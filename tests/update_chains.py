"""Chains of session updates: [(S_0, cfg_0), (d_1, rows_1, S_1, cfg_1), ..., (d_K, rows_K, S_K, cfg_K)], built deterministically from a seed or a script.

kai_session_update / kai_session_update_rows adjust what the open derives (kai_session_update.hpp host_bookkeeping) instead of computing it again, so a quantity
that drifts shows at the second or the tenth update, not at the first.  The chains here walk those quantities: the random ones feed every cycle's outcome into
the next delta as a wrapper that keeps one handle alive does, the scripted ones move ONE cached quantity away, back and away again in small steps.

No test lives here.  tests/test_update_chains.py builds every chain with the oracle as the runner and checks that the chains are worth running;
tests/test_gpu_update_chains.py walks them on the MI355X with the handle under test as the runner.  The runner is `run(snap, cfg, actions)`: whatever it
returns needs `ops` [(kind, pod, node, job)], `pod_status`, `pod_node` and `gpu_groups`, as T.Oracle.run's result has them.
"""
import copy
import functools

import numpy as np

import kai_testlib as T
from test_gpu_session_rows import case as rows_case, random_rows, started_jobs
from test_gpu_session_update import random_delta, session_case

pkg = T.pkg
abi = pkg.abi
synth = pkg.synth
CYCLE = ("allocate", "consolidation", "reclaim", "preempt")
S = abi.POD_STATUS
PENDING, ALLOCATED, PIPELINED, BINDING, BOUND, RUNNING, RELEASING, SUCCEEDED, DELETED = (S[k] for k in ("Pending", "Allocated", "Pipelined", "Binding", "Bound", "Running",
                                                                                                         "Releasing", "Succeeded", "Deleted"))
PLACED = ALLOCATED | BINDING | BOUND | RUNNING
SEC = 1_000_000_000
BATCH, ENGINE = True, False  # kai_action_stats.reserved[4] != 0 after the allocate action: the batch path ran it / the sequential engine did


class Item:
    """One element of a chain.  k = 0: the open (delta and rows are None); k >= 1: the update that leads to snap / cfg.  path: the value of the path bit the chain
    expects from the allocate action on this snapshot (None: the chain names none); between: what the device test does between this step's cycle and the next update
    (None, "reset", "query"); state: what a scripted chain says about this snapshot, checked by tests/test_update_chains.py; res: the runner's result of the cycle."""

    def __init__(self, k, delta, rows, snap, cfg, path=None, between=None, state=None):
        self.k, self.delta, self.rows, self.snap, self.cfg, self.path, self.between, self.state, self.res = k, delta, rows, snap, cfg, path, between, state, None

    def as_tuple(self):
        return (self.snap, self.cfg) if self.k == 0 else (self.delta, self.rows, self.snap, self.cfg)


class Chain:
    def __init__(self, name, actions, items, info=None):
        self.name, self.actions, self.items, self.info = name, actions, items, info or {}

    def as_list(self):
        return [it.as_tuple() for it in self.items]


def build(spec, run, on_item=None):
    """The chain of `spec` with the cycles run by `run(snap, cfg, actions)`.  on_item(item) is called for every element before its cycle runs (the device test
    brings its handle to item.snap there).  Every element's cycle runs, the last one's too: item.res holds what the runner returned."""
    items = [spec.first()]
    while True:
        it = items[-1]
        if on_item is not None:
            on_item(it)
        it.res = run(it.snap, it.cfg, spec.actions)
        nxt = spec.after(it)
        if nxt is None:
            return Chain(spec.name, spec.actions, items, getattr(spec, "info", {}))
        d, rows, meta = nxt
        snap, cfg = it.snap, it.cfg
        if d is not None:
            snap = abi.apply_delta(snap, **d)
        if rows is not None:
            snap, cfg = abi.apply_rows(snap, cfg, **rows)
        items.append(Item(it.k + 1, d, rows, snap, cfg, **meta))


def same_delta(a, b):
    """Two deltas (or two sets of rows) with the same keys and equal values."""
    if a is None or b is None:
        return a is None and b is None
    if set(a) != set(b):
        return False
    for k in a:
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))):
            return False
    return True


def canonical_groups(snap):
    """pod_gpu_group with the groups a cycle opened (ids at and above KAI_NEW_GROUP: a UUID in the reference) renamed in order of first appearance over the pods, per
    node: two runners may name them differently (test_engine_hostsim._same_groups allows it), the snapshots they lead to are the same up to these names."""
    g = snap.pod_gpu_group.copy()
    names = {}
    for p in np.nonzero(g >= T.NEW_GPU_GROUP)[0]:
        g[p] = names.setdefault((int(snap.pod_node[p]), int(g[p])), T.NEW_GPU_GROUP + len(names))
    return g


def same_snapshot(s1, s2, group_names=True):
    if s1.n_res != s2.n_res or set(s1.arrays) != set(s2.arrays):
        return False
    skip = set() if group_names else {"pod_gpu_group"}
    if not all(np.array_equal(s1.arrays[k], s2.arrays[k]) for k in s1.arrays if k not in skip):
        return False
    return group_names or "pod_gpu_group" not in s1.arrays or np.array_equal(canonical_groups(s1), canonical_groups(s2))


def same_item(a, b, group_names=True):
    """group_names=False: equal up to the names of the shared-GPU groups that cycles opened (canonical_groups)."""
    da, db = a.delta, b.delta
    if not group_names and da is not None and db is not None and da.get("gpu_group") is not None and db.get("gpu_group") is not None:
        cut = lambda d: dict(d, gpu_group=np.minimum(np.asarray(d["gpu_group"]), T.NEW_GPU_GROUP))
        da, db = cut(da), cut(db)
    return a.k == b.k and same_delta(da, db) and same_delta(a.rows, b.rows) and same_snapshot(a.snap, b.snap, group_names) and bytes(a.cfg) == bytes(b.cfg)


# ------------------------------------------------------------------------------------------------ what the path bit depends on, as far as a snapshot shows it
def has_shared_gpus(snap):
    a = snap.arrays
    return bool(("pod_gpu_portion" in a and (a["pod_gpu_portion"] > 0).any()) or ("pod_gpu_memory" in a and (a["pod_gpu_memory"] > 0).any()))


def predict_path(snap, cfg):
    """BATCH where nothing a snapshot shows keeps the allocate action off the batch path (kai_session_update.hpp rederive(): batch_ok, fast_ok, all_tracked, no shared
    GPUs, at most four resource rows): no Releasing or Pipelined pod, no node or pod quantity that is no integer or whose sums are not exact, no shared GPUs, no MIG
    rows, some pending pod.
    The jobs' own qualification (kai_batch_kernels.hpp kb_qualify: one pod-set, no topology, no elastic gang that runs) is decided on the device and is not part of
    this rule: on a snapshot with such jobs BATCH here is necessary, not sufficient.  The scripted chains name the bit only on shapes whose jobs all qualify."""
    if cfg.engine_mode != 0 or snap.n_res > 4 or has_shared_gpus(snap):
        return ENGINE
    if (snap.pod_status & (RELEASING | PIPELINED)).any() or not (snap.pod_status == PENDING).any():
        return ENGINE
    for x in (snap.node_allocatable, snap.pod_req):
        if (x < 0).any() or (x != np.floor(x)).any():
            return ENGINE
    for r in range(snap.n_res):  # ... and integers whose sums stay exact: per resource below 2 ** 52 of the unit all its quantities share (HostPrep::build_batch)
        unit = 1 << _unit_shift(snap, r)
        if max(sum(snap.node_allocatable[r].astype(np.uint64).tolist()), sum(snap.pod_req[r].astype(np.uint64).tolist())) // unit >= 1 << 52:
            return ENGINE
    return BATCH


def pending_keys(snap):
    """The distinct request keys (request column, predicate class) among the pending pods: what the class table is ranked from."""
    return {(tuple(snap.pod_req[:, p]), int(snap.pod_class[p])) for p in np.nonzero(snap.pod_status == PENDING)[0]}


# ------------------------------------------------------------------------------------------------ the feedback of a cycle into the next delta
def cycle_feedback(snap, res, rng, succeeded_frac=0.03):
    """abi.next_cycle_delta carried on: what the next cycle's snapshot holds for the pods after a cycle with result `res` ran on `snap`.
     * a pod the cycle placed runs at its node; one it pipelined is Pending again (integration_tests_utils.go: the session is rebuilt from what the cluster holds);
     * a pod the cycle evicted is Releasing at its node; a pod that was Releasing in `snap` already is Deleted, node -1;
     * a seeded `succeeded_frac` of the pods that were and stay Running (one at least) is Succeeded, node -1;
     * with shared GPUs a placed fraction pod carries the group the cycle's group read-back names, an evicted one keeps its own, every pod that leaves its node
       gives its group up — so ids at and above KAI_NEW_GROUP enter and leave the snapshot.
    Returns {pod: (status, node, group)}; group is -1 in a session without shared GPUs."""
    st0 = snap.pod_status
    st1, nd1 = np.asarray(res.pod_status), np.asarray(res.pod_node)
    portion = snap.arrays.get("pod_gpu_portion")
    old_group = snap.arrays.get("pod_gpu_group", np.full(snap.n_pods, -1, np.int32))
    new_group = np.asarray(getattr(res, "gpu_groups", np.full(snap.n_pods, -1, np.int32)))
    frac = (lambda p: portion is not None and portion[p] > 0)
    out = {}
    for p in np.nonzero(st0 == RELEASING)[0]:
        out[int(p)] = (DELETED, -1, -1)
    for p in sorted({int(o[1]) for o in res.ops}):
        if p in out:
            continue
        s1 = int(st1[p])
        if s1 == RELEASING:
            out[p] = (RELEASING, int(nd1[p]), int(old_group[p]) if frac(p) else -1)
        elif s1 == PIPELINED:
            out[p] = (PENDING, -1, -1)
        elif s1 & PLACED:
            out[p] = (RUNNING, int(nd1[p]), int(new_group[p]) if frac(p) else -1)
        else:
            out[p] = (s1, int(nd1[p]), -1)
    running = np.array([p for p in np.nonzero(st0 == RUNNING)[0] if int(p) not in out], np.int64)
    if len(running):
        n = max(1, int(len(running) * succeeded_frac))
        for p in rng.choice(running, size=n, replace=False):
            out[int(p)] = (SUCCEEDED, -1, -1)
    return out


def node_part(snap, snap0, rng):
    """The node part of random_delta (cordon bit, allocatable down, now and then a CPU quantity that is no integer), and the way up: a listed node goes back to what
    S_0 held for it every other time, so that counts behind the guards come down as well as go up."""
    d = random_delta(snap, rng, frac_groups=False)
    nodes, alloc = d["nodes"], d["node_allocatable"]
    for i, n in enumerate(nodes):
        if rng.random() < 0.5:
            alloc[:, i] = snap0.node_allocatable[:, n]
    return dict(nodes=nodes, node_flags=d["node_flags"], node_allocatable=alloc)


def pods_delta(entries, shared):
    pods = sorted(entries)
    d = dict(pods=pods, status=[entries[p][0] for p in pods], node=[entries[p][1] for p in pods])
    if shared:
        d["gpu_group"] = [entries[p][2] for p in pods]
    return d


class RandomChain:
    """K updates over session_case(seed): every delta is the cycle's feedback (cycle_feedback) merged with node_part; the steps k with (seed + k) % 3 == 0 carry
    random_rows as well, the others go through kai_session_update.  A pod is listed once: the feedback is the only source of pod entries.  Between cycle and
    update the device test resets on the steps with (seed + k) % 3 == 1 and queries best_nodes / ordered_nodes on those with (seed + k) % 3 == 2."""
    K = 6
    actions = CYCLE

    def __init__(self, seed):
        self.seed, self.name = seed, f"random-{seed}"
        self.rng = np.random.default_rng(7700 + seed)
        self.snap0 = None

    def _between(self, k):
        return (None, "reset", "query")[(self.seed + k) % 3]

    def first(self):
        self.snap0, cfg = session_case(self.seed)
        return Item(0, None, None, self.snap0, abi.copy_config(cfg), between=self._between(0))

    def after(self, it):
        if it.k == self.K:
            return None
        k = it.k + 1
        d = pods_delta(cycle_feedback(it.snap, it.res, self.rng), has_shared_gpus(it.snap))
        d.update(node_part(it.snap, self.snap0, self.rng))
        rows = random_rows(it.snap, it.cfg, self.rng) if (self.seed + k) % 3 == 0 else None
        return d, rows, dict(between=self._between(k))


# Eight seeds of session_case, three of them (5, 14, 17) with seed % 3 == 2: shared GPUs.  tests/test_update_chains.py holds every seed to its conditions; seeds of
# range(20) left out and why are listed there (SKIPPED_SEEDS).
RANDOM_SEEDS = (1, 3, 5, 10, 12, 14, 16, 17)


# ------------------------------------------------------------------------------------------------ scripted chains
class Script:
    """A scripted chain: the open and a list of steps, each a function of the snapshot and configuration before it that returns
    dict(delta=..., rows=..., path=..., between=..., state=...).  The steps do not read the cycle's result: the update discards it, as kai_session_reset does."""

    def __init__(self, name, snap, cfg, actions, steps, path=None, state=None):
        self.name, self.actions, self.steps = name, actions, steps
        self._first = Item(0, None, None, snap, abi.copy_config(cfg), path=path, state=state)

    def first(self):
        return self._first

    def after(self, it):
        if it.k == len(self.steps):
            return None
        s = dict(self.steps[it.k](it.snap, it.cfg))
        return s.pop("delta", None), s.pop("rows", None), s


def _node_cols(snap, nodes, edit):
    """A node delta that sets the allocatable columns of `nodes` to edit(column, node) and leaves the flags alone."""
    cols = np.stack([edit(snap.node_allocatable[:, n].copy(), n) for n in nodes], axis=1)
    return dict(pods=[], status=[], node=[], nodes=list(nodes), node_allocatable=cols)


def _set_row(r, value):
    def edit(col, n):
        col[r] = value(n) if callable(value) else value
        return col
    return edit


def _clock(cfg, seconds=60):
    return dict(now_ns=int(cfg.now_ns) + seconds * SEC)


def _batch_snapshot():
    snap, cfg, _ = synth.config(1, 0.5)
    return copy.deepcopy(snap), cfg


def _pod_free_nodes(snap):
    used = set(int(n) for n in snap.pod_node if n >= 0)
    return [n for n in range(snap.n_nodes) if n not in used]


def guards_cpu_fraction():
    """Guards by count, the class guard and the exact-sum guard together.  synth.config(1, 0.5) takes the batch path (BATCH).  Two nodes get a CPU allocatable that is
    no integer: ENGINE.  One is restored: still ENGINE (a flag in place of the count would say BATCH).  The other is restored: BATCH.
    States: the number of nodes whose CPU allocatable is no integer: 0, 2, 1, 0."""
    snap, cfg = _batch_snapshot()
    a, b = 3, 7
    orig = {n: float(snap.node_allocatable[0, n]) for n in (a, b)}
    steps = [lambda s, c: dict(delta=_node_cols(s, [a, b], _set_row(0, lambda n: orig[n] + 0.5)), path=ENGINE, state=2),
             lambda s, c: dict(delta=_node_cols(s, [a], _set_row(0, orig[a])), rows=_clock(c), path=ENGINE, state=1),
             lambda s, c: dict(delta=_node_cols(s, [b], _set_row(0, orig[b])), path=BATCH, state=0, between="reset")]
    return Script("guards-cpu-fraction", snap, cfg, ("allocate",), steps, path=BATCH, state=0)


def guards_cpu_zero():
    """Guards by count, the class guard alone: a CPU allocatable of 0 is an integer (the exact-sum guard passes) but fails the class guard of the CPU placement
    resource (HostPrep::node_guard_fails), which puts the CPU-only request keys off the class table, and a pending pod outside the table keeps allocate off the batch
    path.  The shape is config(1, 0.5)'s with a fifth of the pods CPU-only.  Two pod-free nodes lose their CPUs: ENGINE; one gets them back: ENGINE; the other: BATCH.
    States: the number of nodes with a CPU allocatable of 0: 0, 2, 1, 0."""
    snap = synth.make_snapshot(500, 5000, synth.SEED0 + 1, queue_levels=(2, 2), prefill=0.3, cpu_only_frac=0.2)
    cfg = abi.default_config()
    assert any(not (k[0][abi.RES_GPU] > 0) for k in pending_keys(snap)), "the shape needs pending CPU-only pods"
    a, b = _pod_free_nodes(snap)[:2]
    orig = {n: float(snap.node_allocatable[0, n]) for n in (a, b)}
    steps = [lambda s, c: dict(delta=_node_cols(s, [a, b], _set_row(0, 0.0)), path=ENGINE, state=2),
             lambda s, c: dict(delta=_node_cols(s, [b], _set_row(0, orig[b])), path=ENGINE, state=1),
             lambda s, c: dict(delta=_node_cols(s, [a], _set_row(0, orig[a])), rows=_clock(c), path=BATCH, state=0)]
    return Script("guards-cpu-zero", snap, cfg, ("allocate",), steps, path=BATCH, state=0)


def _unit_shift(snap, r):
    """The trailing zeros the node and pod quantities of resource r have in common: the exact-sum guard's unit is 2 ** that.  (Integers below 2 ** 63.)"""
    bits = int(np.bitwise_or.reduce(np.concatenate([snap.node_allocatable[r], snap.pod_req[r]]).astype(np.uint64)))
    return (bits & -bits).bit_length() - 1 if bits else 0


def guards_exact_sums():
    """Guards by count, the exact-sum guard's own counts (HostPrep::NodeSum: bad, the counts per bit, the 128-bit sum) on the memory row, which the class guard does
    not read.  Node a holds no pod and an odd number of bytes (the row's unit is one byte), node b is any other.  (1) a's memory stops being an integer and b's memory brings the nodes' sum to exactly 2 ** 52 units:
    ENGINE.  (2) a is restored, the sum stays: ENGINE.  (3) b comes down by one unit, the sum is 2 ** 52 - 1 units: BATCH.  (4) a is no integer again: ENGINE.
    (5) both are what S_0 held: BATCH.  States: (nodes whose memory is no integer, the memory sum of the other nodes in units >= 2 ** 52): (0, F), (1, F), (0, T), (0, F), (1, F), (0, F) — a value that is no integer takes no part in the sum."""
    snap, cfg = _batch_snapshot()
    R = abi.RES_MEM
    a = _pod_free_nodes(snap)[0]
    b = 11 if a != 11 else 12
    snap.arrays["node_allocatable"][R, a] += 1  # an odd number of bytes: the memory row's unit is one byte, and 2 ** 52 units are a value a node can hold
    tz = _unit_shift(snap, R)
    assert tz <= 10, "2 ** 52 units of the memory row must stay below 2 ** 63"
    others = sum(int(v) for n, v in enumerate(snap.node_allocatable[R]) if n != b)
    edge = (1 << (52 + tz)) - others  # b's memory at which the nodes' sum is exactly 2 ** 52 units
    assert float(edge) == edge and float(edge - (1 << tz)) == edge - (1 << tz), "the edge values must be doubles"
    oa, ob = float(snap.node_allocatable[R, a]), float(snap.node_allocatable[R, b])
    steps = [lambda s, c: dict(delta=_node_cols(s, [a, b], _set_row(R, lambda n: oa + 0.5 if n == a else float(edge))), path=ENGINE, state=(1, False)),
             lambda s, c: dict(delta=_node_cols(s, [a], _set_row(R, oa)), path=ENGINE, state=(0, True)),
             lambda s, c: dict(delta=_node_cols(s, [b], _set_row(R, float(edge - (1 << tz)))), rows=_clock(c), path=BATCH, state=(0, False), between="query"),
             lambda s, c: dict(delta=_node_cols(s, [a], _set_row(R, oa + 0.5)), path=ENGINE, state=(1, False)),
             lambda s, c: dict(delta=_node_cols(s, [a, b], _set_row(R, lambda n: oa if n == a else ob)), path=BATCH, state=(0, False))]
    return Script("guards-exact-sums", snap, cfg, ("allocate",), steps, path=BATCH, state=(0, False))


def exact_sums_state(snap):
    """(nodes whose memory is no integer, the nodes' memory sum in units >= 2 ** 52) — guards_exact_sums' states, from the snapshot."""
    m = snap.node_allocatable[abi.RES_MEM]
    whole = m == np.floor(m)
    ints = [int(v) for v in m[whole]]
    bits = 0
    for v in ints + [int(v) for v in snap.pod_req[abi.RES_MEM]]:
        bits |= v
    tz = (bits & -bits).bit_length() - 1 if bits else 0
    return int((~whole).sum()), (sum(ints) >> tz) >= (1 << 52)


def releasing_by_count():
    """Releasing by count (prep.n_relpipe, from k_delta_gather's wave-reduced counter).  Two Running pods go Releasing: ENGINE.  One runs again: still ENGINE.  The
    other runs again: BATCH, and the cycle commits the operations of step 0.  States: the number of Releasing pods: 0, 2, 1, 0."""
    snap, cfg = _batch_snapshot()
    run = np.nonzero(snap.pod_status == RUNNING)[0]
    p, q = int(run[0]), int(run[len(run) // 2])
    at = {x: int(snap.pod_node[x]) for x in (p, q)}
    steps = [lambda s, c: dict(delta=dict(pods=[p, q], status=[RELEASING, RELEASING], node=[at[p], at[q]]), path=ENGINE, state=2),
             lambda s, c: dict(delta=dict(pods=[q], status=[RUNNING], node=[at[q]]), rows=_clock(c, 0), path=ENGINE, state=1, between="reset"),
             lambda s, c: dict(delta=dict(pods=[p], status=[RUNNING], node=[at[p]]), path=BATCH, state=0)]
    return Script("releasing-by-count", snap, cfg, ("allocate",), steps, path=BATCH, state=0)


def class_table():
    """The class table (prep.cfreq, cls_cap, the batch path's pools, d_pkey / d_remap).  The open holds pending pods of ONE request key (the others' are Succeeded, as
    test_gpu_update_class_table_grows has them): cls_cap is 1.  (1) every pod is Pending: the table grows past cls_cap and the pools are bound again.  (2) back to the
    one key: the table shrinks, the pools bound for the large table stay.  (3) a different single key.  (4) all again: the table that shrank grows on the pools of (1).
    States: the number of distinct pending request keys: 1, n, 1, 1, n with n >= 3."""
    full, cfg = _batch_snapshot()
    keys = {}
    for p in np.nonzero(full.pod_status == PENDING)[0]:
        keys.setdefault((tuple(full.pod_req[:, p]), int(full.pod_class[p])), []).append(int(p))
    assert len(keys) >= 3, "the shape needs several request keys among its pending pods"
    order = list(keys)
    first, second = order[0], order[1]
    but = lambda key: sorted(p for k, ps in keys.items() if k != key for p in ps)
    n = len(keys)
    snap = abi.apply_delta(full, but(first), [SUCCEEDED] * len(but(first)), [-1] * len(but(first)))

    def to(key):  # the delta after which exactly `key`'s pods are pending (None: all)
        def step(s, c):
            want = np.full(s.n_pods, False)
            want[[p for k, ps in keys.items() if key is None or k == key for p in ps]] = True
            mine = np.full(s.n_pods, False); mine[[p for ps in keys.values() for p in ps]] = True
            ch = np.nonzero(mine & (want != (s.pod_status == PENDING)))[0]
            return dict(pods=[int(p) for p in ch], status=[PENDING if want[p] else SUCCEEDED for p in ch], node=[-1] * len(ch))
        return step
    steps = [lambda s, c: dict(delta=to(None)(s, c), path=BATCH, state=n),
             lambda s, c: dict(delta=to(first)(s, c), rows=_clock(c), path=BATCH, state=1, between="query"),
             lambda s, c: dict(delta=to(second)(s, c), path=BATCH, state=1),
             lambda s, c: dict(delta=to(None)(s, c), path=BATCH, state=n, between="reset")]
    return Script("class-table", snap, cfg, ("allocate",), steps, path=BATCH, state=1)


DELTA_SIZES = ((1, 0), (255, 3), (256, 1), (257, 3), (3, 1), (1025, 3), (0, 3), (0, 0))  # (pod entries, node entries) of delta_sizes' steps


def delta_sizes():
    """Delta sizes against the 256 threads of a workgroup of k_delta_gather / k_apply_delta: pod entries 1, 255, 256, 257, 3, 1 025 with 0, 1 or 3 node entries behind
    them in one grid — the node section starts inside a workgroup (255 + 3: it also crosses into the next one) and on a boundary (256 + 1) — then 0 pods with 3 nodes,
    then the empty delta.  Every node entry and the LAST pod entries of every delta are real changes (a kernel that drops the tail of its grid shows): whole jobs turn
    Succeeded and come back to what S_0 held, so that every queued job stays a whole gang; a node entry flips the cordon bit and moves the CPU allocatable by one core.  The
    pod entries in front are statuses the snapshot already holds, which is a legal delta.  The path stays BATCH.  States: DELTA_SIZES' pair per step."""
    snap0, cfg = _batch_snapshot()
    rng = np.random.default_rng(4242)
    jobs = [int(j) for j in rng.permutation(snap0.n_jobs) if snap0.job_n_pods[j] > 0]

    def step(i):
        NP, NN = DELTA_SIZES[i]

        def f(s, c):
            pods, st, nd = [], [], []
            for j in jobs[i::3]:  # whole jobs, toggled between S_0's state and Succeeded, as many as fit into half the entries (one at least)
                ps = list(range(int(s.job_first_pod[j]), int(s.job_first_pod[j]) + int(s.job_n_pods[j])))
                if len(pods) + len(ps) > max(NP // 2, min(NP, 1)) and pods:
                    break
                if len(ps) > NP:
                    continue
                gone = s.pod_status[ps[0]] == SUCCEEDED
                pods += ps; st += [int(snap0.pod_status[p]) if gone else SUCCEEDED for p in ps]; nd += [int(snap0.pod_node[p]) if gone else -1 for p in ps]
            listed = set(pods)
            held = [int(p) for p in rng.permutation(s.n_pods) if int(p) not in listed][: NP - len(pods)]
            pods, st, nd = held + pods, [int(s.pod_status[p]) for p in held] + st, [int(s.pod_node[p]) for p in held] + nd
            assert len(pods) == NP
            d = dict(pods=pods, status=st, node=nd)
            if NN:
                nodes = [int(n) for n in rng.choice(s.n_nodes, size=NN, replace=False)]
                cols = s.node_allocatable[:, nodes].copy()
                cols[0] = np.where(cols[0] == snap0.node_allocatable[0, nodes], cols[0] - 1000, snap0.node_allocatable[0, nodes])
                d.update(nodes=nodes, node_flags=[int(s.node_flags[n]) ^ 0x1 for n in nodes], node_allocatable=cols)
            out = dict(delta=d, path=BATCH, state=(NP, NN))
            if i == 2:
                out["rows"] = _clock(c)
            if i in (3, 5):
                out["between"] = ("reset", "query")[i == 5]
            return out
        return f
    return Script("delta-sizes", snap0, cfg, ("allocate",), [step(i) for i in range(len(DELTA_SIZES))], path=BATCH, state=None)


LATE_ARRAYS = ("job_last_start_ns", "queue_preempt_min_runtime_ns", "queue_reclaim_min_runtime_ns")


def rows_appear_late():
    """Rows appear late (the arrays k_apply_rows creates on first use).  The open has no job_last_start_ns and no min-runtime array.  (1) a pod delta, no rows.  (2) the
    first rows: two jobs' last start, two queues' preempt min-runtime — the arrays come into being.  (3) a pod delta only: the arrays must stay.  (4) rows for OTHER
    queues and jobs, the reclaim min-runtime with them.  The whole cycle runs at every step, so the victim actions' replicas are laid out again each time.  The shape
    (the crowded case of seed 6) has jobs the batch path does not take; the chain names no path bit and compares it with the fresh handle's.
    States: which of LATE_ARRAYS the snapshot holds: none, none, the first two, the first two, all three."""
    snap, cfg = rows_case("crowded", 6)
    for k in LATE_ARRAYS:
        del snap.arrays[k]
    Q = snap.n_queues
    js = started_jobs(snap)
    assert len(js) >= 4 and Q >= 4
    run = [int(p) for p in np.nonzero(snap.pod_status == RUNNING)[0]]
    now = int(cfg.now_ns)
    steps = [lambda s, c: dict(delta=dict(pods=[run[0]], status=[SUCCEEDED], node=[-1]), state=()),
             lambda s, c: dict(rows=dict(queues=[1, Q - 1], queue_preempt_min_runtime_ns=[900 * SEC, -1], jobs=[int(js[0]), int(js[-1])],
                                         job_last_start_ns=[now - SEC, now - 2 * SEC]), state=LATE_ARRAYS[:2], between="reset"),
             lambda s, c: dict(delta=dict(pods=[run[1], run[0]], status=[SUCCEEDED, RUNNING], node=[-1, int(snap.pod_node[run[0]])]), state=LATE_ARRAYS[:2]),
             lambda s, c: dict(delta=dict(pods=[run[1]], status=[RUNNING], node=[int(snap.pod_node[run[1]])]),
                               rows=dict(now_ns=now + 60 * SEC, queues=[0, 2], queue_preempt_min_runtime_ns=[0, 600 * SEC], queue_reclaim_min_runtime_ns=[-1, 600 * SEC],
                                         jobs=[int(js[1]), int(js[2])], job_last_start_ns=[now - 3 * SEC, 0]), state=LATE_ARRAYS, between="query")]
    return Script("rows-appear-late", snap, cfg, CYCLE, steps, state=())


def legacy_mig():
    """Legacy MIG (core->legacy_cnt, the `touched` / `extra` nodes and the second node section of scatter()).  On synth.add_mig(config(1, 0.3), 11, legacy_frac=0.5) node
    n runs two legacy MIG tasks (the second one moved there before the open: add_mig leaves one running pod per MIG node) and is cordoned at the open.  Its running legacy tasks go
    2 -> 1 -> 0 -> 1 -> 2 and n is never in the delta's node list, except at the step 2 -> 1, where it is listed with a cordon change (it is ready from then on; the
    legacy bit travels with the delta's own node entry there).  At 1 -> 0 and 1 -> 2 another node is listed, so n's entry lies behind the delta's own in the second node
    section.  With no legacy task left the cycle places MIG requests on n.  MIG rows keep allocate on the sequential engine: ENGINE throughout.
    States: running legacy MIG tasks on n: 2, 1, 0, 1, 2."""
    snap, cfg, _ = synth.config(1, 0.3)
    snap = copy.deepcopy(snap)
    synth.add_mig(snap, 11, legacy_frac=0.5)
    running = (snap.pod_status == RUNNING) & (snap.pod_node >= 0)
    leg = [int(x) for x in np.nonzero(running & ((snap.pod_flags & abi.POD_LEGACY_MIG) != 0))[0]]
    # add_mig leaves one running pod per MIG node: a second legacy task moves to node n before the open, where both fit.  The node must matter: with its legacy tasks
    # gone the cycle places a MIG request there (tests/test_update_chains.py checks it on the chain), so a stale legacy bit changes the operations.  The first such
    # pair in index order.
    n = ps = None
    for p1 in leg:
        m = int(snap.pod_node[p1])
        p2 = next((x for x in leg if x != p1 and (snap.pod_req[:, x] + snap.pod_req[:, p1] <= snap.node_allocatable[:, m]).all()), None)
        if p2 is None:
            continue
        gone = abi.apply_delta(snap, [p1, p2], [SUCCEEDED] * 2, [-1] * 2)
        if any(o[0] == 0 and o[2] == m for o in T.Oracle.run(gone, cfg, ("allocate",)).ops):
            n, ps = m, [p1, p2]
            break
    assert n is not None, "the shape needs two running legacy MIG tasks that fit one node, which the cycle fills once they are gone"
    snap.arrays["pod_node"][ps[1]] = n
    snap.arrays["node_flags"][n] |= abi.NODE_NOT_READY
    snap.finalize()
    p, q = ps[0], ps[1]
    other = next(m for m in range(snap.n_nodes) if m != n)
    steps = [lambda s, c: dict(delta=dict(pods=[p], status=[SUCCEEDED], node=[-1], nodes=[other, n], node_flags=[int(s.node_flags[other]), int(s.node_flags[n]) ^ 0x1]),
                               path=ENGINE, state=1),
             lambda s, c: dict(delta=dict(pods=[q], status=[SUCCEEDED], node=[-1], nodes=[other], node_flags=[int(s.node_flags[other]) ^ 0x1]), path=ENGINE, state=0,
                               between="reset"),
             lambda s, c: dict(delta=dict(pods=[p], status=[RUNNING], node=[n]), rows=_clock(c), path=ENGINE, state=1),
             lambda s, c: dict(delta=dict(pods=[q], status=[RUNNING], node=[n], nodes=[other], node_flags=[int(s.node_flags[other]) ^ 0x1]), path=ENGINE, state=2)]
    sc = Script("legacy-mig", snap, cfg, ("allocate",), steps, path=ENGINE, state=2)
    sc.info = dict(node=n)
    return sc


def legacy_on(snap, n):
    return int(((snap.pod_flags & abi.POD_LEGACY_MIG) != 0)[(snap.pod_node == n) & ((snap.pod_status & abi.ACTIVE_USED) != 0)].sum())


NEW_GROUP = T.NEW_GPU_GROUP


def shared_gpus():
    """Shared GPUs (core->np_lists in UID order, core->new_groups' counts, next_group0).  synth.add_fractions on config(1, 0.2) with pod_uid_rank a seeded permutation, so
    UID order is not index order.  x is a running fraction pod on node A, B another node that runs fraction pods, y one of them (another job's).
    (1) x moves to B into a group of its own, G = KAI_NEW_GROUP.  (2) y leaves B (Succeeded).  (3) x moves back to A into its old group: no new group is left.
    (4) x and y enter ONE new group G + 5 on B.  (5) x leaves it (back to A): the group lives on with y.  (6) y leaves: no new group is left, next_group0 is
    KAI_NEW_GROUP again.  (7) y opens a new group with the id a fresh open would hand out first, KAI_NEW_GROUP.
    Shared GPUs keep allocate on the sequential engine: ENGINE throughout.
    States: (x's node is B, the new group ids in the snapshot with their pod counts): (F, {}), (T, {G: 1}), (T, {G: 1}), (F, {}), (T, {G+5: 2}), (F, {G+5: 1}), (F, {}), (F, {G: 1})."""
    snap, cfg, _ = synth.config(1, 0.2)
    snap = copy.deepcopy(snap)
    synth.add_fractions(snap, 3, frac=0.4)
    uid = np.random.default_rng(3).permutation(snap.n_pods).astype(np.uint32)
    por, grp = snap.pod_gpu_portion, snap.pod_gpu_group
    fr = [int(p) for p in np.nonzero((por > 0) & (snap.pod_status == RUNNING) & (snap.pod_node >= 0))[0]]
    per = {}
    for p in fr:
        per.setdefault(int(snap.pod_node[p]), []).append(p)
    idle = T.Oracle.run(snap, cfg, ()).nodes["idle"][:, abi.RES_GPU]  # B needs a free device for the group x opens there
    A = min(per)
    x = per[A][0]
    B, y = next((n, p) for n in sorted(per) if n != A and idle[n] >= 1 for p in per[n] if snap.pod_job[p] != snap.pod_job[x] and por[p] + por[x] <= 1.0)
    # x is the first pod of the cluster in UID order: in B's list it belongs in front of B's own pods, not behind them
    first = int(np.nonzero(uid == 0)[0][0])
    uid[first], uid[x] = uid[x], 0
    snap.arrays["pod_uid_rank"] = uid
    snap.finalize()
    gx = int(grp[x])
    G = NEW_GROUP
    one = lambda pod, st, nd, g: dict(pods=[pod], status=[st], node=[nd], gpu_group=[g])
    steps = [lambda s, c: dict(delta=one(x, RUNNING, B, G), path=ENGINE, state=(True, {G: 1})),
             lambda s, c: dict(delta=one(y, SUCCEEDED, -1, -1), path=ENGINE, state=(True, {G: 1}), between="reset"),
             lambda s, c: dict(delta=one(x, RUNNING, A, gx), rows=_clock(c), path=ENGINE, state=(False, {})),
             lambda s, c: dict(delta=dict(pods=[y, x], status=[RUNNING, RUNNING], node=[B, B], gpu_group=[G + 5, G + 5]), path=ENGINE, state=(True, {G + 5: 2})),
             lambda s, c: dict(delta=one(x, RUNNING, A, gx), path=ENGINE, state=(False, {G + 5: 1}), between="query"),
             lambda s, c: dict(delta=one(y, SUCCEEDED, -1, -1), path=ENGINE, state=(False, {})),
             lambda s, c: dict(delta=one(y, RUNNING, B, G), path=ENGINE, state=(False, {G: 1}))]
    sc = Script("shared-gpus", snap, cfg, ("allocate",), steps, path=ENGINE, state=(False, {}))
    sc.info = dict(x=x, A=A, B=B)
    return sc


def new_groups(snap):
    """The shared-GPU group ids at and above KAI_NEW_GROUP that fraction pods of the snapshot carry, with their pod counts (core->new_groups)."""
    g = snap.pod_gpu_group[(snap.pod_gpu_portion > 0) & (snap.pod_gpu_group >= NEW_GROUP)]
    return {int(k): int(v) for k, v in zip(*np.unique(g, return_counts=True))}


SCRIPTED = (guards_cpu_fraction, guards_cpu_zero, guards_exact_sums, releasing_by_count, class_table, delta_sizes, rows_appear_late, legacy_mig, shared_gpus)


@functools.lru_cache(maxsize=None)
def oracle_chain(key):
    """The chain of a random seed (int) or of a scripted chain (its function's name) with T.Oracle.run as the runner, built once per process."""
    spec = RandomChain(key) if isinstance(key, int) else globals()[key]()
    return build(spec, T.Oracle.run)
