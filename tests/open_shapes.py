"""The smallest sessions at which the session-open, action-init and drain kernels (kai_open_kernels.hpp) can go wrong: a wavefront's lane stride, a partial last
workgroup, the fair-share kernel's two forms, a barrier between two heights of the queue tree.  tests/test_open_kernels.py runs them on the emulator under every
wavefront schedule, tests/test_gpu_open_digest.py holds the MI355X against the emulator on them."""
import numpy as np

import kai_testlib as T

abi, synth = T.pkg.abi, T.pkg.synth
S = abi.POD_STATUS


def _set_queues(snap, parent, job_queue):
    """replace the snapshot's queue tree: `parent` per queue (-1 = top), every leaf deserves an equal share of the GPUs, inner queues the sum of their children"""
    a = snap.arrays
    parent = np.asarray(parent, np.int32); Q = len(parent)
    leaves = np.setdiff1d(np.arange(Q), parent)
    deserved = np.full((3, Q), -1.0)
    deserved[abi.Q_GPU, leaves] = np.floor(a["node_allocatable"][abi.RES_GPU].sum() / len(leaves))
    for q in range(Q - 1, -1, -1):  # (children have higher indices than their parents)
        if parent[q] >= 0:
            deserved[abi.Q_GPU, parent[q]] = max(deserved[abi.Q_GPU, parent[q]], 0.0) + deserved[abi.Q_GPU, q]
    a["queue_parent"] = parent; a["queue_priority"] = np.full(Q, 100, np.int32); a["queue_created_ns"] = (np.arange(Q, dtype=np.int64) + 1) * 60_000_000_000
    a["queue_uid_rank"] = np.arange(Q, dtype=np.uint32); a["queue_deserved"] = deserved; a["queue_limit"] = np.full((3, Q), -1.0)
    a["queue_oqw"] = np.ones((3, Q)); a["queue_usage"] = np.zeros((3, Q)); a["job_queue"] = np.asarray(job_queue, np.int32)
    snap.queue_names = [f"q-{i:05d}" for i in range(Q)]
    return snap.finalize()


def leaf_sizes():
    """leaf queues with 0, 1, 64, 65 and 130 queued jobs (none, a partial, a full, a full and a partial, two full and a partial pass of k_leaf_init's wavefront), every
    seventh job an elastic gang that already runs at (state 1) or above (state 2) its minAvailable: the leaf's side heap"""
    counts = (0, 1, 64, 65, 130)
    snap = synth.make_snapshot(24, 4 * sum(counts), 7001, queue_levels=(1, 5), prefill=0.0, gang_sizes=(4,), gang_p=(1.0,), gpus_per_pod=(1,))
    a = snap.arrays
    assert snap.n_jobs == sum(counts) and (a["job_n_pods"] == 4).all()
    a["job_queue"] = np.repeat(np.arange(1, 6, dtype=np.int32), counts)
    n = 0
    for j in range(0, snap.n_jobs, 7):
        b = int(a["job_first_pod"][j]); running = 2 + (j // 7) % 2  # of 4 pods, minAvailable 2: exactly / above
        a["podset_min_available"][a["job_first_podset"][j]] = 2
        a["pod_status"][b:b + running] = S["Running"]; a["pod_node"][b:b + running] = n % snap.n_nodes; n += 1
    return snap.finalize(), abi.default_config()


def tall_tree():
    """a queue tree of four heights (leaves, 120 inner queues, 2 top queues, the root): 120 x 9 fields are more than k_tree_usage's 1 024 threads, and the top
    queues' sums read what the height below them wrote"""
    snap = synth.make_snapshot(40, 500, 7002, queue_levels=(2, 60, 2), prefill=0.3)
    return snap, abi.default_config(k_value=0.5)


def sibling_sets():
    """three top queues with 1, 64 and 65 children: k_fair_share_level's LDS form at its smallest and largest set and the form above 64, on levels of 1 and 3
    sibling sets (3 and 9 wavefronts: no multiple of the workgroup's 4)"""
    snap = synth.make_snapshot(30, 400, 7003, queue_levels=(1, 1), prefill=0.3)
    parent = [-1, -1, -1] + [0] + [1] * 64 + [2] * 65
    rng = np.random.default_rng(7003)
    return _set_queues(snap, parent, rng.integers(3, len(parent), size=snap.n_jobs)), abi.default_config(k_value=0.5)


def node_counts(n_nodes):
    """N nodes (1, 64, 65, 100: a partial block, NB no multiple of a workgroup's 4 wavefronts) with nodes that are not ready, pods of another scheduler, pending pods
    (node -1), and P no multiple of 256"""
    snap = synth.make_snapshot(n_nodes, 3 * n_nodes + 7, 7100 + n_nodes, queue_levels=(2, 2), prefill=0.5, gpus_per_pod=(1, 2))
    synth.add_predicate_features(snap, 7100 + n_nodes, not_ready_frac=0.2, foreign_frac=0.5, nominated_frac=0.0, oversized_frac=0.0)
    a = snap.arrays
    assert snap.n_pods % 256 and (a["pod_node"] < 0).any()
    if n_nodes >= 64:
        on = a["pod_node"][a["pod_node"] >= 0]
        assert (a["node_flags"][on] & abi.NODE_NOT_READY).any() and (a["pod_flags"] & abi.POD_FOREIGN_SCHEDULER).any()
    return snap, abi.default_config()


def shared_gpus():
    """shared GPUs: four fraction pods on each of three nodes, their UID order not their index order (k_node_accounting_shared walks np_pods); portions that are
    exact in binary, so the queue sums do not depend on the order of addition"""
    snap = synth.make_snapshot(4, 40, 7004, queue_levels=(1, 2), prefill=0.0, single_pod_jobs=True)
    a = snap.arrays
    a["pod_status"][:12] = S["Running"]; a["pod_node"][:12] = np.arange(12) % 3
    synth.add_fractions(snap, 7004, frac=1.0, portions=(0.25, 0.5))
    a = snap.arrays
    assert (a["pod_gpu_portion"][:12] > 0).all()
    a["pod_uid_rank"] = np.random.default_rng(7004).permutation(snap.n_pods).astype(np.uint32)
    return snap.finalize(), abi.default_config()


def shapes():
    """(name, snapshot, config, shared GPUs in the session)"""
    yield ("leaf sizes",) + leaf_sizes() + (False,)
    yield ("tall tree",) + tall_tree() + (False,)
    yield ("sibling sets",) + sibling_sets() + (False,)
    for n in (1, 64, 65, 100):
        yield (f"{n} nodes",) + node_counts(n) + (False,)
    yield ("shared GPUs",) + shared_gpus() + (True,)
