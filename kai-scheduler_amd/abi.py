"""ctypes mirror of include/kai_core.h and the structure-of-arrays session snapshot.

`Snapshot` is the host-side twin of the reference's `api.ClusterInfo` (pkg/scheduler/api/cluster_info.go:43-64)
already flattened to the arrays `kai_snapshot_soa` carries.  Strings never cross the ABI: names are ranked
once here (byte-wise order, like Go's string compare) because the reference's tie-breaks are string compares
(framework/session.go:480-485, session_plugins.go:227-260).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

KAI_ABI_VERSION = 5
RES_CPU, RES_MEM, RES_GPU, RES_PODS = 0, 1, 2, 3
MAX_RES = 8
Q_CPU, Q_MEM, Q_GPU = 0, 1, 2
UNLIMITED = -1.0

# pod status bit-set (api/pod_status/pod_status.go:25-71)
POD_STATUS = {
    "Pending": 1 << 0, "Gated": 1 << 1, "Allocated": 1 << 2, "Pipelined": 1 << 3, "Binding": 1 << 4, "Bound": 1 << 5,
    "Running": 1 << 6, "Releasing": 1 << 7, "Succeeded": 1 << 8, "Failed": 1 << 9, "Unknown": 1 << 10, "Deleted": 1 << 11,
}
POD_STATUS_NAME = {v: k for k, v in POD_STATUS.items()}
ACTIVE_USED = sum(POD_STATUS[s] for s in ("Allocated", "Pipelined", "Binding", "Bound", "Running", "Releasing"))

NODE_NOT_READY, NODE_MIG_ENABLED, NODE_MIG_MIXED, NODE_HAS_DRA_GPUS, NODE_GPU_WORKER, NODE_CPU_WORKER, NODE_MIG_SINGLE = 1, 2, 4, 8, 16, 32, 64
POD_FOREIGN_SCHEDULER, POD_HAS_TASK_PRIORITY, POD_CPU_FALLBACK, POD_GPU_UNMODELLED, POD_LEGACY_MIG = 1, 2, 4, 8, 16

ACTIONS = {"allocate": 0, "consolidation": 1, "reclaim": 2, "preempt": 3}
OP_KIND = {0: "allocate", 1: "pipeline", 2: "evict"}
BINPACK, SPREAD = 0, 1
PLUGINS = {"predicates": 0x001, "proportion": 0x002, "priority": 0x004, "elastic": 0x008, "nodeavailability": 0x010,
           "resourcetype": 0x020, "subgrouporder": 0x040, "taskorder": 0x080, "nominatednode": 0x100, "nodeplacement": 0x200,
           "minruntime": 0x400, "topology": 0x800, "gpusharingorder": 0x1000, "gpupack": 0x2000, "gpuspread": 0x4000}
PLUGIN_PREDICATES, PLUGIN_PROPORTION, PLUGIN_PRIORITY, PLUGIN_ELASTIC, PLUGIN_NODEAVAILABILITY, PLUGIN_RESOURCETYPE = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
PLUGIN_SUBGROUPORDER, PLUGIN_TASKORDER, PLUGIN_NOMINATEDNODE, PLUGIN_NODEPLACEMENT, PLUGIN_MINRUNTIME, PLUGIN_TOPOLOGY = 0x040, 0x080, 0x100, 0x200, 0x400, 0x800
PLUGIN_ALL = 0x3FFF  # the default tier list (conf_util/scheduler_conf_util.go:36-61): everything except gpuspread

STATUS_TEXT = {0: "ok", -1: "invalid argument", -2: "no HIP device", -3: "HIP runtime error", -4: "output capacity",
               -5: "unsupported snapshot feature", -6: "call order", -7: "device engine fault", -8: "multi-GPU exchange", -9: "out of host memory"}


class KaiConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("gpu_strategy", C.c_int32), ("cpu_strategy", C.c_int32), ("k_value", C.c_double),
        ("reclaimer_saturation_multiplier", C.c_double), ("plugins", C.c_uint32), ("restrict_node_scheduling", C.c_int32),
        ("max_consolidation_preemptees", C.c_int32), ("use_scheduling_signatures", C.c_int32), ("allow_consolidating_reclaim", C.c_int32),
        ("full_hierarchy_fairness", C.c_int32), ("min_node_gpu_memory", C.c_int64), ("queue_depth", C.c_int32 * 4),
        ("engine_mode", C.c_int32), ("reserved", C.c_int32 * 7),
        ("now_ns", C.c_int64), ("default_preempt_min_runtime_ns", C.c_int64), ("default_reclaim_min_runtime_ns", C.c_int64),
        ("reclaim_resolve_method", C.c_int32), ("pad0", C.c_int32),
    ]


def default_config(**kw) -> KaiConfig:
    """Defaults of conf_util/scheduler_conf_util.go:36-61 + conf/scheduler_conf.go:31-46."""
    c = KaiConfig()
    c.abi_version = KAI_ABI_VERSION
    c.gpu_strategy = BINPACK
    c.cpu_strategy = BINPACK
    c.k_value = 1.0
    c.reclaimer_saturation_multiplier = 1.0
    c.plugins = PLUGIN_ALL
    c.restrict_node_scheduling = 0
    c.max_consolidation_preemptees = 16
    c.use_scheduling_signatures = 1
    c.allow_consolidating_reclaim = 1
    c.full_hierarchy_fairness = 1
    c.min_node_gpu_memory = 100
    for i in range(4):
        c.queue_depth[i] = -1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


_P = C.POINTER


class KaiSnapshotSoA(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("n_res", C.c_int32),
        ("n_nodes", C.c_int32), ("node_allocatable", _P(C.c_double)), ("node_flags", _P(C.c_uint32)), ("node_gpu_count", _P(C.c_int32)),
        ("node_name_rank", _P(C.c_uint32)), ("node_class", _P(C.c_int32)),
        ("n_pods", C.c_int32), ("pod_req", _P(C.c_double)), ("pod_job", _P(C.c_int32)), ("pod_podset", _P(C.c_int32)),
        ("pod_status", _P(C.c_int32)), ("pod_node", _P(C.c_int32)), ("pod_flags", _P(C.c_uint32)), ("pod_task_priority", _P(C.c_int32)),
        ("pod_created_ns", _P(C.c_int64)), ("pod_uid_rank", _P(C.c_uint32)), ("pod_class", _P(C.c_int32)), ("pod_nominated_node", _P(C.c_int32)),
        ("n_podsets", C.c_int32), ("podset_job", _P(C.c_int32)), ("podset_min_available", _P(C.c_int32)), ("podset_name_rank", _P(C.c_uint32)),
        ("n_jobs", C.c_int32), ("job_queue", _P(C.c_int32)), ("job_priority", _P(C.c_int32)), ("job_preemptible", _P(C.c_int32)),
        ("job_created_ns", _P(C.c_int64)), ("job_uid_rank", _P(C.c_uint32)), ("job_first_pod", _P(C.c_int32)), ("job_n_pods", _P(C.c_int32)),
        ("job_first_podset", _P(C.c_int32)), ("job_n_podsets", _P(C.c_int32)),
        ("n_queues", C.c_int32), ("queue_parent", _P(C.c_int32)), ("queue_priority", _P(C.c_int32)), ("queue_created_ns", _P(C.c_int64)),
        ("queue_uid_rank", _P(C.c_uint32)), ("queue_deserved", _P(C.c_double)), ("queue_limit", _P(C.c_double)), ("queue_oqw", _P(C.c_double)),
        ("queue_usage", _P(C.c_double)),
        ("n_pod_classes", C.c_int32), ("n_node_classes", C.c_int32), ("class_fit", _P(C.c_uint8)),
        ("n_topologies", C.c_int32), ("topo_level_off", _P(C.c_int32)), ("n_topo_levels", C.c_int32), ("node_domain", _P(C.c_int32)),
        ("n_domains", C.c_int32), ("domain_level", _P(C.c_int32)), ("domain_parent", _P(C.c_int32)), ("domain_id_rank", _P(C.c_uint32)),
        ("n_groups", C.c_int32), ("group_job", _P(C.c_int32)), ("group_parent", _P(C.c_int32)), ("group_name_rank", _P(C.c_uint32)),
        ("group_topology", _P(C.c_int32)), ("group_required_level", _P(C.c_int32)), ("group_preferred_level", _P(C.c_int32)),
        ("job_root_group", _P(C.c_int32)), ("podset_group", _P(C.c_int32)), ("podset_topology", _P(C.c_int32)),
        ("podset_required_level", _P(C.c_int32)), ("podset_preferred_level", _P(C.c_int32)),
        ("job_signature", _P(C.c_int64)),
        ("job_last_start_ns", _P(C.c_int64)), ("queue_preempt_min_runtime_ns", _P(C.c_int64)), ("queue_reclaim_min_runtime_ns", _P(C.c_int64)),
        ("pod_gpu_portion", _P(C.c_double)), ("pod_gpu_group", _P(C.c_int32)), ("node_gpu_memory", _P(C.c_int64)), ("pod_gpu_memory", _P(C.c_int64)),
        ("res_mig_gpus", _P(C.c_int32)), ("res_mig_memory", _P(C.c_int64)),
    ]


DELTA_VERSION = 1  # KAI_DELTA_VERSION


class KaiSessionDelta(C.Structure):
    """kai_session_delta (include/kai_core.h): pod and node changes applied to the open session by kai_session_update."""
    _fields_ = [("version", C.c_uint32), ("n_pods", C.c_int32), ("pod", C.POINTER(C.c_int32)), ("pod_status", C.POINTER(C.c_int32)),
                ("pod_node", C.POINTER(C.c_int32)), ("pod_gpu_group", C.POINTER(C.c_int32)), ("n_nodes", C.c_int32), ("node", C.POINTER(C.c_int32)),
                ("node_flags", C.POINTER(C.c_uint32)), ("node_allocatable", C.POINTER(C.c_double))]


def apply_delta(snap: "Snapshot", pods, status, node, gpu_group=None, nodes=None, node_flags=None, node_allocatable=None) -> "Snapshot":
    """S' = S with a kai_session_delta applied: a new Snapshot (arrays the delta touches are copied, the others shared) that kai_session_open accepts.
    node_allocatable is [R][len(nodes)], as in the C struct."""
    a = dict(snap.arrays)
    pods = np.asarray(pods, np.int64)
    if len(pods):
        a["pod_status"] = a["pod_status"].copy(); a["pod_status"][pods] = np.asarray(status, np.int32)
        a["pod_node"] = a["pod_node"].copy(); a["pod_node"][pods] = np.asarray(node, np.int32)
        if gpu_group is not None:
            g = a["pod_gpu_group"].copy() if "pod_gpu_group" in a else np.full(snap.n_pods, -1, np.int32)
            g[pods] = np.asarray(gpu_group, np.int32); a["pod_gpu_group"] = g
    if nodes is not None and len(nodes):
        nodes = np.asarray(nodes, np.int64)
        if node_flags is not None:
            a["node_flags"] = a["node_flags"].copy(); a["node_flags"][nodes] = np.asarray(node_flags, np.uint32)
        if node_allocatable is not None:
            a["node_allocatable"] = a["node_allocatable"].copy(); a["node_allocatable"][:, nodes] = np.asarray(node_allocatable, np.float64).reshape(snap.n_res, len(nodes))
    out = Snapshot(n_res=snap.n_res, arrays=a, node_names=snap.node_names, pod_names=snap.pod_names, job_names=snap.job_names,
                   queue_names=snap.queue_names, podset_names=snap.podset_names)
    out.finalize()
    return out


ROWS_VERSION = 1  # KAI_ROWS_VERSION
ROWS_HAS_NOW = 0x1


class KaiSessionRows(C.Structure):
    """kai_session_rows (include/kai_core.h): the cycle's clock, queue rows and job start times applied by kai_session_update_rows."""
    _fields_ = [("version", C.c_uint32), ("fields", C.c_uint32), ("now_ns", C.c_int64), ("n_queues", C.c_int32), ("queue", C.POINTER(C.c_int32)),
                ("queue_deserved", C.POINTER(C.c_double)), ("queue_limit", C.POINTER(C.c_double)), ("queue_oqw", C.POINTER(C.c_double)),
                ("queue_usage", C.POINTER(C.c_double)), ("queue_priority", C.POINTER(C.c_int32)), ("queue_preempt_min_runtime_ns", C.POINTER(C.c_int64)),
                ("queue_reclaim_min_runtime_ns", C.POINTER(C.c_int64)), ("n_jobs", C.c_int32), ("job", C.POINTER(C.c_int32)),
                ("job_last_start_ns", C.POINTER(C.c_int64))]


def copy_config(cfg: KaiConfig) -> KaiConfig:
    out = KaiConfig()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(KaiConfig))
    return out


def apply_rows(snap: "Snapshot", cfg: KaiConfig, now_ns=None, queues=None, queue_deserved=None, queue_limit=None, queue_oqw=None, queue_usage=None,
               queue_priority=None, queue_preempt_min_runtime_ns=None, queue_reclaim_min_runtime_ns=None, jobs=None, job_last_start_ns=None):
    """(S', cfg') = (S, cfg) with a kai_session_rows applied: a new Snapshot (the arrays the rows touch are copied, the others shared) and a new KaiConfig that
    kai_core_create / kai_session_open accept.  The four queue quantities are [3][len(queues)], as in the C struct.  An optional array the snapshot lacks and the
    rows carry for at least one row is created with the value an absent array stands for (0 for queue_usage and job_last_start_ns, -1 for the min-runtimes)."""
    a = dict(snap.arrays)
    cfg2 = copy_config(cfg)
    if now_ns is not None:
        cfg2.now_ns = int(now_ns)
    Q, J = snap.n_queues, snap.n_jobs

    def put(name, idx, val, shape, dt, absent):
        if val is None or not len(idx):
            return
        arr = a[name].copy() if name in a else np.full(shape, absent, dt)
        if arr.ndim == 2:
            arr[:, idx] = np.asarray(val, dt).reshape(3, len(idx))
        else:
            arr[idx] = np.asarray(val, dt)
        a[name] = arr
    qi = np.asarray([] if queues is None else queues, np.int64)
    ji = np.asarray([] if jobs is None else jobs, np.int64)
    put("queue_deserved", qi, queue_deserved, (3, Q), np.float64, 0.0)
    put("queue_limit", qi, queue_limit, (3, Q), np.float64, 0.0)
    put("queue_oqw", qi, queue_oqw, (3, Q), np.float64, 0.0)
    put("queue_usage", qi, queue_usage, (3, Q), np.float64, 0.0)
    put("queue_priority", qi, queue_priority, (Q,), np.int32, 0)
    put("queue_preempt_min_runtime_ns", qi, queue_preempt_min_runtime_ns, (Q,), np.int64, -1)
    put("queue_reclaim_min_runtime_ns", qi, queue_reclaim_min_runtime_ns, (Q,), np.int64, -1)
    put("job_last_start_ns", ji, job_last_start_ns, (J,), np.int64, 0)
    out = Snapshot(n_res=snap.n_res, arrays=a, node_names=snap.node_names, pod_names=snap.pod_names, job_names=snap.job_names,
                   queue_names=snap.queue_names, podset_names=snap.podset_names)
    out.finalize()
    return out, cfg2


def next_cycle_delta(snap: "Snapshot", ops, rng, succeeded_frac=0.01) -> dict:
    """The delta a real next cycle carries after a cycle's operations `ops` (kai_op records): the allocated pods Running at their nodes, the pipelined ones
    Pending, and `succeeded_frac` of the running pods Succeeded.  Keyword arguments of apply_delta / Session.update (pods, status, node)."""
    placed = {int(o["pod"]): int(o["node"]) for o in ops if int(o["kind"]) == 0}
    piped = [int(o["pod"]) for o in ops if int(o["kind"]) == 1 and int(o["pod"]) not in placed]
    running = np.nonzero(snap.pod_status == 1 << 6)[0]
    k = int(len(running) * succeeded_frac)
    done = [int(p) for p in rng.choice(running, size=k, replace=False) if int(p) not in placed] if k else []
    pods = list(placed) + piped + done
    status = [1 << 6] * len(placed) + [1] * len(piped) + [1 << 8] * len(done)
    node = list(placed.values()) + [-1] * (len(piped) + len(done))
    return dict(pods=pods, status=status, node=node)


class KaiOp(C.Structure):
    _fields_ = [("seq", C.c_int64), ("kind", C.c_int32), ("pod", C.c_int32), ("node", C.c_int32), ("job", C.c_int32), ("stmt", C.c_int32), ("pad", C.c_int32)]


QUERY_PIPELINE_ONLY = 0x1  # KAI_QUERY_PIPELINE_ONLY
ORDERED_MAX_K = 64         # KAI_ORDERED_MAX_K: the longest list kai_ordered_nodes returns per task


class KaiNodeQuery(C.Structure):
    """kai_node_query (include/kai_core.h): one task of kai_best_nodes; nodeset = a row of the call's bitmaps, -1 = all nodes."""
    _fields_ = [("pod", C.c_int32), ("nodeset", C.c_int32), ("flags", C.c_uint32), ("pad", C.c_int32)]


class KaiNodeAnswer(C.Structure):
    _fields_ = [("node", C.c_int32), ("is_pipeline", C.c_int32)]


APPLY_CHECK_ONLY, APPLY_ENGINE_PATH = 0x1, 0x2          # KAI_APPLY_CHECK_ONLY, KAI_APPLY_ENGINE_PATH
APPLY_PATH_NONE, APPLY_PATH_WIDE, APPLY_PATH_ENGINE = 0, 1, 2  # kai_apply_result.path


class KaiApplyResult(C.Structure):
    """kai_apply_result (include/kai_core.h): what kai_ops_apply says about a batch — the first offending operation (-1 = none), the path that took it, its Statements."""
    _fields_ = [("first_bad", C.c_int64), ("path", C.c_int32), ("statements", C.c_int32)]


STMT_VERSION = 1  # KAI_STMT_VERSION


class KaiStmtResult(C.Structure):
    """kai_stmt_result (include/kai_core.h): what a kai_stmt_* call says — the first offending operation (-1 = none), the log's length after the call, the path that took it."""
    _fields_ = [("first_bad", C.c_int64), ("log_len", C.c_int64), ("path", C.c_int32), ("pad", C.c_int32)]


PLACE_VERSION, PLACE_PIPELINE_ONLY = 1, 0x4  # KAI_PLACE_VERSION, KAI_PLACE_PIPELINE_ONLY (beside APPLY_ENGINE_PATH)
PLACE_PLACED, PLACE_NO_FIT = 0, 1            # kai_place_answer.status


class KaiPlaceParams(C.Structure):
    """kai_place_params (include/kai_core.h): kai_stmt_place's flags."""
    _fields_ = [("version", C.c_uint32), ("flags", C.c_uint32)]


class KaiPlaceGang(C.Structure):
    """kai_place_gang: a gang's tasks (a range of the call's pod list, in placement order), its node sets (a range of the call's set list, in the order they are tried;
    an entry is a row of the node-set bitmaps or -1 = all nodes) and its row of the score rows / deciles (-1 = none)."""
    _fields_ = [("first_task", C.c_int32), ("n_tasks", C.c_int32), ("first_set", C.c_int32), ("n_sets", C.c_int32), ("scores", C.c_int32), ("pad", C.c_int32)]


class KaiPlaceAnswer(C.Structure):
    """kai_place_answer: status (PLACE_*), the set of the gang's own list that took it (-1), the sets tried, and its surviving operations in the call's ops."""
    _fields_ = [("status", C.c_int32), ("set", C.c_int32), ("sets_tried", C.c_int32), ("pad", C.c_int32), ("first_op", C.c_int64), ("n_ops", C.c_int64)]


STALE_VERSION, STALE_DRY_RUN = 1, 0x1  # KAI_STALE_VERSION, KAI_STALE_DRY_RUN


class KaiStaleParams(C.Structure):
    """kai_stale_params (include/kai_core.h): kai_stale_gang_eviction's grace period (negative: never evict) and flags."""
    _fields_ = [("version", C.c_uint32), ("flags", C.c_uint32), ("grace_ns", C.c_int64)]


class KaiStaleResult(C.Structure):
    """kai_stale_result (include/kai_core.h): the stale jobs, those whose grace period ran out, the evictions, the apply path (APPLY_PATH_*) that took them."""
    _fields_ = [("stale_jobs", C.c_int32), ("expired_jobs", C.c_int32), ("n_ops", C.c_int64), ("path", C.c_int32), ("pad", C.c_int32)]


JOB_ORDER_VERSION, JOB_ORDER_ENGINE_PATH = 1, 0x1  # KAI_JOB_ORDER_VERSION, KAI_JOB_ORDER_ENGINE_PATH
JOB_ORDER_PATH_NONE, JOB_ORDER_PATH_WIDE, JOB_ORDER_PATH_ENGINE = 0, 1, 2  # kai_job_order_result.path


class KaiJobOrderParams(C.Structure):
    """kai_job_order_params (include/kai_core.h): kai_job_order's flags and queue depth (0: the config's allocate depth, -1: infinite, > 0: jobs per leaf queue)."""
    _fields_ = [("version", C.c_uint32), ("flags", C.c_uint32), ("depth", C.c_int32), ("pad", C.c_int32)]


class KaiJobOrderResult(C.Structure):
    """kai_job_order_result (include/kai_core.h): the ordered jobs, the path (JOB_ORDER_PATH_*) that ordered them, the leaf queues with a job in the order."""
    _fields_ = [("n_ordered", C.c_int32), ("path", C.c_int32), ("n_leaves", C.c_int32), ("pad", C.c_int32)]


SUBSET_VERSION, SUBSET_ENGINE_PATH = 1, 0x1  # KAI_SUBSET_VERSION, KAI_SUBSET_ENGINE_PATH
SUBSET_PATH_NONE, SUBSET_PATH_WIDE, SUBSET_PATH_ENGINE = 0, 1, 2  # kai_subset_result.path
SUBSET_PARENT = -1  # KAI_SUBSET_PARENT: kai_node_set.domain of "the parent node set as it is"
SUBSET_OK, SUBSET_NO_TOPOLOGY, SUBSET_NO_FIT, SUBSET_BAD_LEVEL = 0, 1, 2, 3  # kai_subset_answer.status
SUBSET_STATUS_TEXT = {SUBSET_OK: "node sets", SUBSET_NO_TOPOLOGY: "the requested topology does not exist", SUBSET_NO_FIT: "no domain can take the tasks",
                      SUBSET_BAD_LEVEL: "no level given, or a level the topology does not have"}


def subset_root(t: int) -> int:
    """KAI_SUBSET_ROOT(t): kai_node_set.domain of the root domain of topology t"""
    return -2 - t


class KaiSubsetParams(C.Structure):
    """kai_subset_params (include/kai_core.h): kai_subset_nodes' flags."""
    _fields_ = [("version", C.c_uint32), ("flags", C.c_uint32)]


class KaiSubsetQuery(C.Structure):
    """kai_subset_query: a job, its SubGroupSet (group) or pod-set (podset) or -1 / -1 for the root, and the parent node-set row (-1: all nodes)."""
    _fields_ = [("job", C.c_int32), ("group", C.c_int32), ("podset", C.c_int32), ("nodeset", C.c_int32)]


class KaiSubsetAnswer(C.Structure):
    """kai_subset_answer: status (SUBSET_*), the number of node sets and where they start, len(tasks), the common domain."""
    _fields_ = [("status", C.c_int32), ("n_sets", C.c_int32), ("first", C.c_int32), ("tasks", C.c_int32), ("common_domain", C.c_int32), ("pad", C.c_int32)]


class KaiNodeSet(C.Structure):
    """kai_node_set: one node set — its domain (or subset_root(t), or SUBSET_PARENT), level, AllocatablePods (-1: not set) and size."""
    _fields_ = [("domain", C.c_int32), ("level", C.c_int32), ("allocatable_pods", C.c_int32), ("n_nodes", C.c_int32)]


class KaiSubsetResult(C.Structure):
    """kai_subset_result: the node sets of all queries and the path (SUBSET_PATH_*) that found them."""
    _fields_ = [("n_sets", C.c_int64), ("path", C.c_int32), ("pad", C.c_int32)]


TOPO_SCORE_UNIT = 10000.0                         # KAI_TOPO_SCORE_UNIT: scores.Topology, a node's score is decile x this
TOPO_NO_SCORE = 255                               # KAI_TOPO_NO_SCORE: decile of a domain whose nodes have no score
TOPO_SCORES_NONE, TOPO_SCORES_EMPTY = -1, -2      # kai_topo_score_row.level_row: no scores left for the sub-group / recorded, but no node has one


class KaiTopoScoreRow(C.Structure):
    """kai_topo_score_row: the node_domain row a node's domain is read from (or TOPO_SCORES_NONE / _EMPTY) and the number of scored domains."""
    _fields_ = [("level_row", C.c_int32), ("n_scored", C.c_int32)]


class KaiScoredQuery(C.Structure):
    """kai_scored_query: kai_node_query with `scores`, the row of the call's score rows / deciles (-1 = none), in place of pad."""
    _fields_ = [("pod", C.c_int32), ("nodeset", C.c_int32), ("flags", C.c_uint32), ("scores", C.c_int32)]


class KaiQueueShare(C.Structure):
    _fields_ = [(n, C.c_double * 3) for n in ("fair_share", "allocated", "allocated_non_preemptible", "request", "deserved", "max_allowed")]


class KaiNodeState(C.Structure):
    _fields_ = [("idle", C.c_double * MAX_RES), ("releasing", C.c_double * MAX_RES), ("used", C.c_double * MAX_RES)]


class KaiActionStats(C.Structure):
    _fields_ = [("decisions", C.c_int64), ("node_scans", C.c_int64), ("nodes_scanned", C.c_int64), ("jobs_attempted", C.c_int64),
                ("jobs_committed", C.c_int64), ("rollbacks", C.c_int64), ("kernel_ms", C.c_double), ("upload_ms", C.c_double),
                ("reserved", C.c_int64 * 8)]


def rank_strings(names) -> np.ndarray:
    """Rank of each string in byte-wise ascending order (Go's `<` on strings); ties keep first-seen order."""
    order = sorted(range(len(names)), key=lambda i: (names[i].encode("utf-8"), i))
    rank = np.empty(len(names), dtype=np.uint32)
    for r, i in enumerate(order):
        rank[i] = r
    return rank


_SPEC = [  # (field, dtype, shape-kind)
    ("node_allocatable", np.float64, "RN"), ("node_flags", np.uint32, "N"), ("node_gpu_count", np.int32, "N"),
    ("node_name_rank", np.uint32, "N"), ("node_class", np.int32, "N"),
    ("pod_req", np.float64, "RP"), ("pod_job", np.int32, "P"), ("pod_podset", np.int32, "P"), ("pod_status", np.int32, "P"),
    ("pod_node", np.int32, "P"), ("pod_flags", np.uint32, "P"), ("pod_task_priority", np.int32, "P"), ("pod_created_ns", np.int64, "P"),
    ("pod_uid_rank", np.uint32, "P"), ("pod_class", np.int32, "P"), ("pod_nominated_node", np.int32, "P"),
    ("podset_job", np.int32, "S"), ("podset_min_available", np.int32, "S"), ("podset_name_rank", np.uint32, "S"),
    ("job_queue", np.int32, "J"), ("job_priority", np.int32, "J"), ("job_preemptible", np.int32, "J"), ("job_created_ns", np.int64, "J"),
    ("job_uid_rank", np.uint32, "J"), ("job_first_pod", np.int32, "J"), ("job_n_pods", np.int32, "J"), ("job_first_podset", np.int32, "J"),
    ("job_n_podsets", np.int32, "J"),
    ("queue_parent", np.int32, "Q"), ("queue_priority", np.int32, "Q"), ("queue_created_ns", np.int64, "Q"), ("queue_uid_rank", np.uint32, "Q"),
    ("queue_deserved", np.float64, "3Q"), ("queue_limit", np.float64, "3Q"), ("queue_oqw", np.float64, "3Q"), ("queue_usage", np.float64, "3Q"),
    ("class_fit", np.uint8, "CF"),
]
# optional topology + sub-group-tree arrays (kai_core.h): present only when the snapshot carries them
_SPEC_OPT = [
    ("topo_level_off", np.int32), ("node_domain", np.int32), ("domain_level", np.int32), ("domain_parent", np.int32), ("domain_id_rank", np.uint32),
    ("group_job", np.int32), ("group_parent", np.int32), ("group_name_rank", np.uint32), ("group_topology", np.int32),
    ("group_required_level", np.int32), ("group_preferred_level", np.int32), ("job_root_group", np.int32), ("podset_group", np.int32),
    ("podset_topology", np.int32), ("podset_required_level", np.int32), ("podset_preferred_level", np.int32),
    ("job_signature", np.int64), ("job_last_start_ns", np.int64), ("queue_preempt_min_runtime_ns", np.int64), ("queue_reclaim_min_runtime_ns", np.int64),
    ("pod_gpu_portion", np.float64), ("pod_gpu_group", np.int32), ("node_gpu_memory", np.int64), ("pod_gpu_memory", np.int64), ("res_mig_gpus", np.int32), ("res_mig_memory", np.int64),
]


@dataclass
class Snapshot:
    """numpy-backed kai_snapshot_soa.  2-D arrays are resource-major ([R][N])."""
    n_res: int = 4
    arrays: dict = field(default_factory=dict)
    # optional name tables (never cross the ABI; for tests / reporting)
    node_names: list = field(default_factory=list)
    pod_names: list = field(default_factory=list)
    job_names: list = field(default_factory=list)
    queue_names: list = field(default_factory=list)
    podset_names: list = field(default_factory=list)

    def __getattr__(self, k):
        arrays = self.__dict__.get("arrays", {})
        if k in arrays:
            return arrays[k]
        raise AttributeError(k)

    @property
    def n_nodes(self): return int(self.arrays["node_flags"].shape[0])
    @property
    def n_pods(self): return int(self.arrays["pod_job"].shape[0])
    @property
    def n_podsets(self): return int(self.arrays["podset_job"].shape[0])
    @property
    def n_jobs(self): return int(self.arrays["job_queue"].shape[0])
    @property
    def n_queues(self): return int(self.arrays["queue_parent"].shape[0])
    @property
    def n_pod_classes(self): return int(self.arrays["class_fit"].shape[0])
    @property
    def n_node_classes(self): return int(self.arrays["class_fit"].shape[1])

    def finalize(self):
        """Coerce dtypes / contiguity and fill optional arrays with their neutral defaults."""
        a = self.arrays
        N, P = self.n_nodes, self.n_pods
        a.setdefault("node_gpu_count", np.full(N, -1, np.int32))
        a.setdefault("node_class", np.zeros(N, np.int32))
        a.setdefault("pod_flags", np.zeros(P, np.uint32))
        a.setdefault("pod_task_priority", np.zeros(P, np.int32))
        a.setdefault("pod_created_ns", np.zeros(P, np.int64))
        a.setdefault("pod_class", np.zeros(P, np.int32))
        a.setdefault("pod_nominated_node", np.full(P, -1, np.int32))
        a.setdefault("class_fit", np.ones((1, 1), np.uint8))
        a.setdefault("queue_usage", np.zeros((3, self.n_queues), np.float64))
        for name, dt, _ in _SPEC:
            a[name] = np.ascontiguousarray(a[name], dtype=dt)
        for name, dt in _SPEC_OPT:
            if name in a:
                a[name] = np.ascontiguousarray(a[name], dtype=dt)
        assert a["node_allocatable"].shape == (self.n_res, N), a["node_allocatable"].shape
        assert a["pod_req"].shape == (self.n_res, P), a["pod_req"].shape
        return self

    def as_struct(self) -> KaiSnapshotSoA:
        a = self.arrays
        s = KaiSnapshotSoA()
        s.abi_version = KAI_ABI_VERSION
        s.n_res = self.n_res
        s.n_nodes, s.n_pods, s.n_podsets, s.n_jobs, s.n_queues = self.n_nodes, self.n_pods, self.n_podsets, self.n_jobs, self.n_queues
        s.n_pod_classes, s.n_node_classes = self.n_pod_classes, self.n_node_classes
        ctype = {np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32, np.dtype(np.uint32): C.c_uint32,
                 np.dtype(np.int64): C.c_int64, np.dtype(np.uint8): C.c_uint8}
        for name, dt, _ in _SPEC:
            arr = a[name]
            setattr(s, name, arr.ctypes.data_as(_P(ctype[np.dtype(dt)])))
        for name, dt in _SPEC_OPT:
            if name in a:
                setattr(s, name, a[name].ctypes.data_as(_P(ctype[np.dtype(dt)])))
        s.n_topologies = int(a["topo_level_off"].shape[0]) - 1 if "topo_level_off" in a else 0
        s.n_topo_levels = int(a["topo_level_off"][-1]) if "topo_level_off" in a else 0
        s.n_domains = int(a["domain_level"].shape[0]) if "domain_level" in a else 0
        s.n_groups = int(a["group_job"].shape[0]) if "group_job" in a else 0
        s._keepalive = a  # the struct borrows the numpy buffers
        return s
