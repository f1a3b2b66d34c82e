/*
 * kai_core.h — C ABI of libkai_core, the MI355X-native scheduling-cycle core.
 *
 * This is the drop-in boundary for the reference's hot path.  A cgo shim on the
 * reference side implements framework.Action (pkg/scheduler/framework/interface.go:41-47) for
 * allocate|consolidation|reclaim|preempt and one framework.Plugin (interface.go:49-55) whose
 * OnSessionOpen packs cache.Snapshot() (pkg/scheduler/cache/cluster_info/cluster_info.go:118-228)
 * into kai_snapshot_soa and calls kai_session_open.  See INTEGRATION.md for the binding.
 *
 * Conventions
 *  - every function returns 0 (KAI_OK) or a negative kai_status; nothing throws, nothing calls back.
 *  - one caller thread per handle; a handle is not re-entrant; several handles may coexist.
 *  - all input buffers are caller-owned host memory (C.malloc'd on the Go side; cgo forbids keeping
 *    Go pointers) and may be freed when the call returns: the library copies them to HBM.
 *  - output buffers are caller-allocated, with a capacity argument.
 *  - indices, not names: the host ranks every string once (node names, UIDs, pod-set names) in
 *    byte-wise order and passes the rank, because the reference's tie-breaks are string compares
 *    (framework/session.go:480-485 node name; session_plugins.go:227-260 UID).
 *  - all quantities are float64 exactly as the reference holds them: cpu in milli-cores, memory in
 *    bytes, gpu in devices, pods as a count (api/resource_info/resource_vector.go:23-36).
 */
#ifndef KAI_CORE_H
#define KAI_CORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KAI_ABI_VERSION 5u

/* resource vector layout: api/resource_info/resource_vector.go:23-36 (cpu, memory, gpu, pods, extras…) */
#define KAI_RES_CPU 0
#define KAI_RES_MEM 1
#define KAI_RES_GPU 2
#define KAI_RES_PODS 3
#define KAI_MAX_RES 8

/* quota resources of the proportion plugin, in its fixed iteration order
 * (plugins/proportion/resource_share/resource_quantities.go:20) */
#define KAI_Q_CPU 0
#define KAI_Q_MEM 1
#define KAI_Q_GPU 2
#define KAI_Q_NRES 3

#define KAI_UNLIMITED (-1.0) /* pkg/common/constants/constants.go:11 */

typedef enum kai_status {
    KAI_OK = 0,
    KAI_ERR_INVALID_ARG = -1,
    KAI_ERR_NO_DEVICE = -2,     /* no usable HIP device: the library never computes on the CPU */
    KAI_ERR_HIP = -3,           /* a HIP runtime call failed (see kai_last_error) */
    KAI_ERR_CAPACITY = -4,      /* an output buffer is too small */
    KAI_ERR_UNSUPPORTED = -5,   /* snapshot needs a feature outside the device path (see kai_pod_flags) */
    KAI_ERR_STATE = -6,         /* call order violated (e.g. action before session_open) */
    KAI_ERR_DEVICE_FAULT = -7,  /* the device engine reported an internal fault / spin timeout */
    KAI_ERR_COMM = -8,          /* multi-GPU exchange failed */
    KAI_ERR_NO_MEMORY = -9      /* host memory ran out while a session was prepared (std::bad_alloc): not a malformed snapshot */
} kai_status;

/* pod status bit-set: api/pod_status/pod_status.go:25-71 */
typedef enum kai_pod_status {
    KAI_POD_PENDING = 1 << 0,
    KAI_POD_GATED = 1 << 1,
    KAI_POD_ALLOCATED = 1 << 2,
    KAI_POD_PIPELINED = 1 << 3,
    KAI_POD_BINDING = 1 << 4,
    KAI_POD_BOUND = 1 << 5,
    KAI_POD_RUNNING = 1 << 6,
    KAI_POD_RELEASING = 1 << 7,
    KAI_POD_SUCCEEDED = 1 << 8,
    KAI_POD_FAILED = 1 << 9,
    KAI_POD_UNKNOWN = 1 << 10,
    KAI_POD_DELETED = 1 << 11
} kai_pod_status;

/* node flag bits (host pre-evaluates the per-node booleans the predicates read) */
#define KAI_NODE_NOT_READY 0x1u      /* scheduler_util/scheduler_utils.go:12-40 says "not fit" */
#define KAI_NODE_MIG_ENABLED 0x2u    /* api/node_info/node_info.go:704-718 */
#define KAI_NODE_MIG_MIXED 0x4u      /* MigStrategy == mixed (node_info.go:720-732) */
#define KAI_NODE_HAS_DRA_GPUS 0x8u   /* node_info.go:95 HasDRAGPUs */
#define KAI_NODE_GPU_WORKER 0x10u    /* has conf GPUWorkerNodeLabelKey (plugins/predicates/predicates.go:243-259) */
#define KAI_NODE_CPU_WORKER 0x20u    /* has conf CPUWorkerNodeLabelKey */
#define KAI_NODE_MIG_SINGLE 0x40u    /* MigStrategy == single (node_info.go:720-732): only whole-GPU tasks may run there (:349-352) */

/* pod flag bits */
#define KAI_POD_FOREIGN_SCHEDULER 0x1u /* spec.schedulerName != ours: plugins/proportion/proportion.go:276-285 */
#define KAI_POD_HAS_TASK_PRIORITY 0x2u /* carries the task-order label: plugins/taskorder/task_order.go:28-63 */
#define KAI_POD_LEGACY_MIG 0x10u       /* PodInfo.IsLegacyMIGtask (pod_info.go:500-516): never schedulable (node_info.go:317-320); a node that holds one takes no MIG request (:342-346) */
#define KAI_POD_CPU_FALLBACK 0x4u      /* needs a state-dependent upstream predicate, fractional GPU, MIG, DRA …:
                                          not placed by the device path (SURVEY §8b fallback rule) */
#define KAI_POD_GPU_UNMODELLED 0x8u    /* holds / asks for GPU state the device's node accounting does not carry (gpu-memory request, several fractional
                                          devices, MIG profile, DRA claim): an ACTIVE pod of that kind would leave its node's idle GPUs overstated
                                          (api/node_info/node_info.go:457-493 addSharedTaskResources), so kai_session_open refuses the snapshot */

typedef enum kai_action {
    KAI_ACTION_ALLOCATE = 0,      /* actions/allocate/allocate.go:46-77 */
    KAI_ACTION_CONSOLIDATION = 1, /* actions/consolidation/consolidation.go:32-78 */
    KAI_ACTION_RECLAIM = 2,       /* actions/reclaim/reclaim.go:47-100 */
    KAI_ACTION_PREEMPT = 3        /* actions/preempt/preempt.go:46-97 */
} kai_action;

typedef enum kai_op_kind {
    KAI_OP_ALLOCATE = 0, /* framework/statement.go:297-358  → cache.Bind on commit  */
    KAI_OP_PIPELINE = 1, /* framework/statement.go:197-295  → cache.TaskPipelined   */
    KAI_OP_EVICT = 2     /* framework/statement.go:63-126   → cache.Evict           */
} kai_op_kind;

typedef enum kai_placement_strategy { KAI_BINPACK = 0, KAI_SPREAD = 1 } kai_placement_strategy;

/* plugins of the default tier that register callbacks on the path (conf_util/scheduler_conf_util.go:39-60).
 * A plugin that is absent registers nothing: its order fn / predicate / score simply does not run. */
#define KAI_PLUGIN_PREDICATES 0x001u
#define KAI_PLUGIN_PROPORTION 0x002u
#define KAI_PLUGIN_PRIORITY 0x004u
#define KAI_PLUGIN_ELASTIC 0x008u
#define KAI_PLUGIN_NODEAVAILABILITY 0x010u
#define KAI_PLUGIN_RESOURCETYPE 0x020u
#define KAI_PLUGIN_SUBGROUPORDER 0x040u
#define KAI_PLUGIN_TASKORDER 0x080u
#define KAI_PLUGIN_NOMINATEDNODE 0x100u
#define KAI_PLUGIN_NODEPLACEMENT 0x200u
#define KAI_PLUGIN_MINRUNTIME 0x400u
#define KAI_PLUGIN_TOPOLOGY 0x800u
/* shared-GPU plugins (fractions of one device, ABI v4): plugins/gpusharingorder (node order), plugins/gpupack and plugins/gpuspread (GPU order inside a node) */
#define KAI_PLUGIN_GPUSHARINGORDER 0x1000u
#define KAI_PLUGIN_GPUPACK 0x2000u
#define KAI_PLUGIN_GPUSPREAD 0x4000u
#define KAI_PLUGIN_ALL 0x3FFFu /* the default tier list: everything above except gpuspread */

/* knobs of conf.SchedulerParams / plugin arguments that the path reads
 * (conf/scheduler_conf.go:31-61, plugins/proportion/proportion.go:67-93,
 *  plugins/nodeplacement/nodeplacement.go:33-47) */
typedef struct kai_config {
    uint32_t abi_version;
    int32_t gpu_strategy;                 /* kai_placement_strategy */
    int32_t cpu_strategy;
    double k_value;                       /* proportion kValue (<=0 → 0) */
    double reclaimer_saturation_multiplier;
    uint32_t plugins;                     /* KAI_PLUGIN_* bit-set: which plugins of the tier list are loaded */
    int32_t restrict_node_scheduling;
    int32_t max_consolidation_preemptees; /* -1 = unlimited */
    int32_t use_scheduling_signatures;
    int32_t allow_consolidating_reclaim;
    int32_t full_hierarchy_fairness;
    int64_t min_node_gpu_memory;          /* ClusterInfo.MinNodeGPUMemory */
    int32_t queue_depth[4];               /* per kai_action; -1 = infinite (framework/session.go:398-404) */
    int32_t engine_mode;                  /* 0 = default (allocate: batch plan/fill/apply path when the action qualifies, else the sequential engine);
                                             1 = force brute-force node scans; 2 = class index without the staged job path; 3 = sequential engine only (debug / A-B).
                                             The batch path's fill runs on sets of nodes by free devices when every scan class is placed on the GPU and asks for a whole number
                                             of 1 .. 16 devices and no other resource of a node can bind before its devices do — under gpu_strategy = KAI_BINPACK, and under
                                             KAI_SPREAD when, besides, every node with a free device carries ONE device count (nvidia.com/gpu.count, else allocatable) and no
                                             class needs a node bitmap of its own; every other session runs the general fill kernel.  Same results either way. */
    int32_t reserved[7];
    /* minruntime plugin (plugins/minruntime/minruntime.go:40-100): "now" of the cycle, plugin-argument defaults, reclaim resolve method */
    int64_t now_ns;                       /* the FIRST cycle's clock: kai_core_set_now / kai_session_rows.now_ns move it on the same handle */
    int64_t default_preempt_min_runtime_ns;
    int64_t default_reclaim_min_runtime_ns;
    int32_t reclaim_resolve_method;       /* 0 = lca (default), 1 = queue */
    int32_t pad0;
} kai_config;

/* Structure-of-arrays session snapshot.  [R][N] means resource-major: element (r, i) at r*N + i. */
typedef struct kai_snapshot_soa {
    uint32_t abi_version;
    int32_t n_res; /* R, 4..KAI_MAX_RES */

    /* ---- nodes: api/node_info/node_info.go:68-105 ---- */
    int32_t n_nodes;
    const double* node_allocatable;   /* [R][N] status.allocatable */
    const uint32_t* node_flags;       /* [N] KAI_NODE_* (bits 28-31 are ignored: the library keeps flags of its own there) */
    const int32_t* node_gpu_count;    /* [N] nvidia.com/gpu.count label, -1 when absent (node_info.go:619-640) */
    const uint32_t* node_name_rank;   /* [N] rank of the node name, byte-wise ascending, unique */
    const int32_t* node_class;        /* [N] column of class_fit */

    /* ---- pods: api/pod_info/pod_info.go:70-112; pods of one job are contiguous ---- */
    int32_t n_pods;
    const double* pod_req;            /* [R][P] ResReq incl. pods:=1 (pod_info.go:373-393) */
    const int32_t* pod_job;           /* [P] */
    const int32_t* pod_podset;        /* [P] global pod-set index */
    const int32_t* pod_status;        /* [P] kai_pod_status */
    const int32_t* pod_node;          /* [P] node index or -1 */
    const uint32_t* pod_flags;        /* [P] KAI_POD_* flag bits */
    const int32_t* pod_task_priority; /* [P] value of the task-order label (valid with KAI_POD_HAS_TASK_PRIORITY) */
    const int64_t* pod_created_ns;    /* [P] Pod.CreationTimestamp */
    const uint32_t* pod_uid_rank;     /* [P] rank of the pod UID, unique */
    const int32_t* pod_class;         /* [P] row of class_fit */
    const int32_t* pod_nominated_node;/* [P] node index of status.nominatedNodeName or -1 */

    /* ---- pod-sets (gang sub-groups): api/podgroup_info/subgroup_info/podset.go:17-29 ---- */
    int32_t n_podsets;
    const int32_t* podset_job;           /* [S] */
    const int32_t* podset_min_available; /* [S] */
    const uint32_t* podset_name_rank;    /* [S] rank of the pod-set name inside its job */

    /* ---- jobs (PodGroups): api/podgroup_info/job_info.go:65-103 ---- */
    int32_t n_jobs;
    const int32_t* job_queue;         /* [J] leaf queue index, -1 if the queue does not exist */
    const int32_t* job_priority;      /* [J] */
    const int32_t* job_preemptible;   /* [J] 0/1 (pkg/common/podgroup/preemptible.go:10-26) */
    const int64_t* job_created_ns;    /* [J] */
    const uint32_t* job_uid_rank;     /* [J] unique */
    const int32_t* job_first_pod;     /* [J] */
    const int32_t* job_n_pods;        /* [J] */
    const int32_t* job_first_podset;  /* [J] */
    const int32_t* job_n_podsets;     /* [J] */

    /* ---- queues: api/queue_info/queue_info.go:32-43 ---- */
    int32_t n_queues;
    const int32_t* queue_parent;      /* [Q] -1 for top queues */
    const int32_t* queue_priority;    /* [Q] */
    const int64_t* queue_created_ns;  /* [Q] */
    const uint32_t* queue_uid_rank;   /* [Q] unique */
    const double* queue_deserved;     /* [3][Q] quota; cpu milli, memory in 10^6-byte units as in the CRD, gpu devices; -1 unlimited */
    const double* queue_limit;        /* [3][Q] */
    const double* queue_oqw;          /* [3][Q] over-quota weight */
    const double* queue_usage;        /* [3][Q] normalised historical usage (api/queue_info/quota_info.go) */

    /* ---- static predicate classes (upstream kube-scheduler Filters pre-evaluated by the host) ---- */
    int32_t n_pod_classes;
    int32_t n_node_classes;
    const uint8_t* class_fit;         /* [n_pod_classes][n_node_classes] 1 = every static Filter passes */

    /* ---- topologies (Topology CR: ordered spec.levels[].nodeLabel; plugins/topology/topology_plugin.go:57-110).
     * Levels of topology t are the global level rows topo_level_off[t] .. topo_level_off[t+1]-1, top level first.  A domain is one
     * distinct prefix of level label values (plugins/topology/topology_structs.go:94-101); the host builds the domain table.
     * All of this may be absent (n_topologies = 0). ---- */
    int32_t n_topologies;
    const int32_t* topo_level_off;    /* [T+1] */
    int32_t n_topo_levels;            /* = topo_level_off[T] */
    const int32_t* node_domain;       /* [n_topo_levels][N] domain of the node at that level, -1 at every level of a topology the node is not
                                         part of (a node joins a topology only if it has every level label: topology/common.go:70-77) */
    int32_t n_domains;
    const int32_t* domain_level;      /* [D] global level row */
    const int32_t* domain_parent;     /* [D] domain at the level above, -1 for a top-level domain */
    const uint32_t* domain_id_rank;   /* [D] rank of the domain ID string ("zone1.rack3") inside its topology, byte-wise ascending */

    /* ---- sub-group tree of every job (api/podgroup_info/subgroup_info/subgroupset.go): groups = SubGroupSets incl. each job's root;
     * pod-sets are the leaves.  Absent (n_groups = 0) ⇒ every job has a root group without constraint holding all its pod-sets.
     * A topology constraint (api/topology_info) is {topology index or -1 (none) or -2 (named topology does not exist),
     * required level, preferred level} with levels counted inside the topology (0 = top) or -1. ---- */
    int32_t n_groups;
    const int32_t* group_job;         /* [G] */
    const int32_t* group_parent;      /* [G] parent group, -1 for the job's root */
    const uint32_t* group_name_rank;  /* [G] rank of the SubGroupSet name inside its job (framework/session_plugins.go:273-282) */
    const int32_t* group_topology;    /* [G] */
    const int32_t* group_required_level;
    const int32_t* group_preferred_level;
    const int32_t* job_root_group;    /* [J] */
    const int32_t* podset_group;      /* [S] parent group of the pod-set */
    const int32_t* podset_topology;   /* [S] the pod-set's own constraint */
    const int32_t* podset_required_level;
    const int32_t* podset_preferred_level;

    /* ---- scheduling-constraints signature (api/podgroup_info/job_info.go:547-570, api/pod_info/scheduling_constraints_signature.go) ----
     * [J] any injective id of the job's signature (the reference hashes node selector, affinity, tolerations, priority class, ...).
     * Only equality is used (actions/common/minimal_job_comparison.go:15-44).  NULL: the victim actions refuse to run with
     * use_scheduling_signatures set. */
    const int64_t* job_signature;

    /* ---- minruntime plugin inputs (all optional; NULL = nothing is protected) ----
     * PodGroupInfo.LastStartTimestamp (ns since the epoch, 0 = never started) and the queues' preemptMinRuntime / reclaimMinRuntime
     * (ns, -1 = not set on that queue; resolved up the tree, plugins/minruntime/resolver.go:33-190) */
    const int64_t* job_last_start_ns;            /* [J] */
    const int64_t* queue_preempt_min_runtime_ns; /* [Q] */
    const int64_t* queue_reclaim_min_runtime_ns; /* [Q] */

    /* ---- fractional GPU requests (ABI v4; all optional, NULL = no pod asks for a fraction) ----
     * pod_gpu_portion: 0 = a whole-GPU or CPU-only pod; in (0, 1) = a fraction of ONE device (annotation gpu-fraction,
     *   api/pod_info/pod_info.go:472-477); pod_req's gpu column then holds ResourceRequirements.GPUs() of it: the portion rounded to 1/100
     *   (fixed point, api/resource_info/gpu_resource_requirment.go:230-234) — 0.125 counts as 0.13 against quota, and as int64(0.125 * memory) on the device.
     * pod_gpu_group: the shared-GPU group an ACTIVE fraction pod runs in (label runai-gpu-group; PodInfo.GPUGroups), as an id >= 0 that is
     *   unique on its node; -1 = none.  Equality on one node is what the accounting uses (api/node_info/gpu_sharing_node_info.go); in addition
     *   ids below 2^20 stand for numeric group names and ids from 2^20 on for any other name, because the predicates plugin takes a
     *   non-numeric name for a group that is being created (plugins/predicates/predicates.go:320-330).
     * node_gpu_memory: NodeInfo.MemoryOfEveryGpuOnNode in MiB (label nvidia.com/gpu.memory floored to a multiple of 100, node_info.go:673-687);
     *   NULL = 100 on every node (DefaultGpuMemory).
     * pod_gpu_memory (ABI v5): > 0 = the pod asks for that many MiB of ONE device (annotation gpu-memory, pod_info.go:463-468): its gpu
     *   column in pod_req and its pod_gpu_portion are 0 (ResourceRequirements.GPUs() of such a request is 0); on a node it takes that memory of a
     *   shared device and counts as ceil(memory / node_gpu_memory * 100) / 100 of a device (node_info.go:329-332, 661-666, 734-744); while pending it
     *   weighs memory / kai_config.min_node_gpu_memory in its queue's request and in its job's resources (proportion.go:360-366,
     *   allocation_info.go:103-107).  NULL = no such pod. */
    const double* pod_gpu_portion;   /* [P] */
    const int32_t* pod_gpu_group;    /* [P] */
    const int64_t* node_gpu_memory;  /* [N] */
    const int64_t* pod_gpu_memory;   /* [P] */

    /* ---- MIG profiles (ABI v5; optional, NULL = no resource row is a MIG profile) ----
     * A MIG instance type (nvidia.com/mig-<g>g.<m>gb) is a resource row >= 4 of node_allocatable / pod_req, counted in instances.  res_mig_gpus[r] = g (its GPU
     * weight, api/common_info/resources/mig.go:13-33), 0 for every other row; res_mig_memory[r] = m.  A pod that requests such a row is a MIG request
     * (RequestTypeMigInstance, pod_info.go:493-497): its GPU quota is sum(g x instances) while ResourceRequirements.GPUs() stays 0
     * (gpu_resource_requirment.go:163-178); nodes count idle instances by their weight (resource_info.go:177-194, node_info.go:592-628); the predicates
     * of api/node_info/node_info.go:315-359 apply (KAI_NODE_MIG_* flags, KAI_POD_LEGACY_MIG). */
    const int32_t* res_mig_gpus;     /* [R] */
    const int64_t* res_mig_memory;   /* [R] */
} kai_snapshot_soa;

typedef struct kai_op {
    int64_t seq;   /* position in commit order */
    int32_t kind;  /* kai_op_kind */
    int32_t pod;
    int32_t node;
    int32_t job;   /* the pod's own job */
    int32_t stmt;  /* Statement the operation was committed by (framework/statement.go:536-575), numbered from 0 per action in commit order:
                      the shim replays the operations of one id through ONE Statement — a reclaim statement is "evict A, evict B, pipeline C" */
    int32_t pad;
} kai_op;

/* per queue, in KAI_Q_* order: plugins/proportion/resource_share/resource_share.go:12-21 */
typedef struct kai_queue_share {
    double fair_share[KAI_Q_NRES];
    double allocated[KAI_Q_NRES];
    double allocated_non_preemptible[KAI_Q_NRES];
    double request[KAI_Q_NRES];
    double deserved[KAI_Q_NRES];
    double max_allowed[KAI_Q_NRES];
} kai_queue_share;

typedef struct kai_node_state {
    double idle[KAI_MAX_RES];
    double releasing[KAI_MAX_RES];
    double used[KAI_MAX_RES];
} kai_node_state;

/* engine statistics of the last kai_action_execute (measurement) */
typedef struct kai_action_stats {
    int64_t decisions;          /* allocateTask executions (ended in allocate / pipeline / fail) */
    int64_t node_scans;         /* full passes over a node set */
    int64_t nodes_scanned;      /* Σ node-set sizes over those passes */
    int64_t jobs_attempted;
    int64_t jobs_committed;
    int64_t rollbacks;
    double kernel_ms;           /* HIP-event time of the action kernel on its stream */
    double upload_ms;           /* snapshot → HBM (session_open only) */
    int64_t reserved[8];        /* [0] index queries, [1] block refreshes / loads, [2] drained jobs | scenarios, [3] drained decisions | simulations,
                                   [4] rounds of the batch path (0 = sequential engine), [5..7] cycle / time counters of the path that ran (kai_core.hip).
                                   Victim actions (consolidation / reclaim / preempt): [1] workgroups the action ran on (default 32, environment KAI_VICTIM_WGS;
                                   1 with shared GPUs in the session), [5] waves of simulations, [6] simulations run << 32 | simulations the reference's order reaches.
                                   Allocate on the sequential engine of a cluster of >= 1024 nodes: bits 48.. of [1] = workgroups that took the passes over the nodes
                                   (scan grid: the engine's own + the helpers; default 16 launched, 32 from 4096 nodes, environment KAI_SCAN_WGS, 1 = off) */
} kai_action_stats;

typedef struct kai_core kai_core; /* opaque */

/* replaces: scheduler.NewScheduler wiring (pkg/scheduler/scheduler.go:53-101); gpu_ids = HIP device ordinals.
 * n_gpus == 1: the whole session on gpu_ids[0].  n_gpus > 1: ONE PROCESS PER GPU — this handle is one rank of a group of n_gpus handles that
 * shard the NODE axis of one session (contiguous name-rank ranges; pods, jobs, queues replicated) on the GPUs of one node; gpu_ids[0] is this
 * rank's device and kai_shard_attach names the rank and the group's all-gather.  Every rank opens the same snapshot and makes the same calls. */
int kai_core_create(const kai_config* cfg, int n_gpus, const int* gpu_ids, kai_core** out);

/* The group's exchange step: an all-gather of `bytes_per_rank` bytes from every rank's `send` into `recv` (rank-major), on DEVICE
 * memory of the library.  The library has no communicator of its own: the caller supplies the collective (the Python mirror:
 * torch.distributed.all_gather_into_tensor over RCCL / xGMI) and the library calls it between kernels, with its stream synchronised.
 * offers_per_class: nodes a rank offers per scan class and exchange (0 = default 128).  Returns 0 / a kai_status. */
typedef int (*kai_allgather_fn)(void* user, const void* send, void* recv, int64_t bytes_per_rank);
int kai_shard_attach(kai_core* core, int rank, int world, int offers_per_class, kai_allgather_fn fn, void* user);
/* Victim actions (reclaim, preempt, consolidation) on a group: every rank holds the whole session, the SIMULATIONS of a partial job are dealt out over the ranks
 * (simulation i of a wave to rank i mod n_gpus; the reference's loop: actions/common/solvers/job_solver.go:95-126, by_pod_solver.go:61-144) and a wave ends with one
 * all-gather of its outcomes (68 bytes per simulation).  That exchange happens while the action's kernel is running and waits for it, so it is the host's: `fn` is
 * called from inside kai_action_execute with HOST memory of the library and must not synchronise the device (the kernel only goes on when fn has returned).
 * Without it — and without the library's own communicator below — a group runs its victim actions replicated (same results, nothing shortened). */
int kai_shard_attach_host(kai_core* core, kai_allgather_fn fn, void* user);
/* The same exchange from the library itself: its own RCCL communicator (librccl is resolved at run time), the all-gather issued on the library's stream between the
 * kernels it separates — no host round trip, no staging.  Rank 0 draws the 128-byte id (ncclGetUniqueId), the caller carries it to the other ranks by whatever it has
 * (the Python mirror: torch.distributed.broadcast), every rank attaches with it (ncclCommInitRank: collective over the group, one device per rank).
 * kai_shard_allgather_probe runs the group's exchange step once on caller-provided device buffers (diagnostics; what the fill calls between kernels). */
#define KAI_RCCL_ID_BYTES 128
int kai_shard_rccl_id(kai_core* core, void* id_out /* KAI_RCCL_ID_BYTES */);
int kai_shard_attach_rccl(kai_core* core, int rank, int world, int offers_per_class, const void* id /* KAI_RCCL_ID_BYTES, the same on every rank */);
int kai_shard_allgather_probe(kai_core* core, const void* send, void* recv, int64_t bytes_per_rank);
int kai_core_destroy(kai_core* core);

/* replaces: framework.OpenSession + every OnSessionOpen on the path (framework/framework.go:32-65):
 * node accounting from the pods (api/node_info/node_info.go:457-493), proportion totals / queue usage /
 * fair-share division (plugins/proportion/proportion.go:242-423).
 * The snapshot's arrays are read during the call only.  The handle keeps what it derives from them on the host (name-rank permutation, job lists, scan
 * classes: about 150 bytes per pod) and its device slabs for the next open, as a scheduler opens a session per cycle (scheduler.go:112-138); kai_core_destroy
 * releases both.  The loops of the preparation run on a process-wide pool of worker threads (KAI_HOST_THREADS, KAI_HOST_POOL: INTEGRATION.md). */
int kai_session_open(kai_core* core, const kai_snapshot_soa* snap);

/* Re-opens the session from the snapshot copy that is already resident in HBM (no host traffic): same math as
 * kai_session_open.  Lets a caller replay scheduling cycles on one snapshot (benchmarks, what-if runs). */
int kai_session_reset(kai_core* core);

/* A pod and node delta applied to the open session's snapshot: what changes between two scheduling cycles of a live cluster (the pods the last cycle placed go
 * Binding -> Running, pipelined / evicted ones go back to Pending or Releasing, a few finish or are deleted, a few nodes are cordoned, go NotReady or change
 * allocatable).  Indices are the snapshot's (the caller's order); NULL optional arrays leave that quantity unchanged.
 *
 * Contract.  Let S be the snapshot of the last kai_session_open or kai_session_update and S' be S with the delta applied.  After KAI_OK the handle is
 * indistinguishable from one that has just run kai_session_open(S'): the same kai_queue_shares, kai_node_states, kai_pod_states and kai_pod_gpu_groups, bit for
 * bit, and the same operations, states, shares, groups and decision counters from every action run afterwards (the batch path or the sequential engine included,
 * kai_action_stats.reserved[4]).  The update applies to the snapshot, not to the state the actions left: it discards their results as kai_session_reset does,
 * and kai_session_reset afterwards returns to S'.
 *  - KAI_ERR_INVALID_ARG: a wrong version, an index out of range (a pod, a node, a pod_node other than -1 .. n_nodes-1), a pod or node listed twice,
 *    a NULL required array with a count above 0;
 *  - KAI_ERR_STATE: no open session;
 *  - KAI_ERR_UNSUPPORTED: a handle of a sharded group (n_gpus > 1); a delta kai_session_open(S') would refuse (e.g. a KAI_POD_GPU_UNMODELLED pod made active,
 *    a KAI_POD_CPU_FALLBACK pod made pending, a node that gains GPUs with another node_gpu_memory in a session with shared-GPU requests), with the open's
 *    status; and, in such a session, a delta after which every node that has GPUs is a new one with another memory size, or none is left while the caller's
 *    node 0 has another one (the cluster's GPU memory size would change, and every fraction's memory with it: open S').
 *  Every refusal is decided before the first write and leaves the session exactly as it was (still open, same snapshot, same state); only a HIP failure after
 *  the writes began closes it, as a failed open does.  The host work is proportional to the delta (plus, in a session with shared-GPU requests, one pass over
 *  the nodes' lists of active pods); the session math is re-derived on the device as kai_session_reset does.
 *  Anything the delta and the rows below cannot express needs a full open: pods, jobs, pod-sets, queues or nodes added or removed; job_priority,
 *  job_preemptible, job_queue; queue_parent, queue_created_ns, queue_uid_rank; requests, classes, class_fit, topologies; any kai_config field other
 *  than now_ns. */
#define KAI_DELTA_VERSION 1u
typedef struct kai_session_delta {
    uint32_t version;                /* KAI_DELTA_VERSION */
    int32_t n_pods;                  /* pods whose state changed */
    const int32_t* pod;              /* [n_pods] pod index in the snapshot's (caller's) order */
    const int32_t* pod_status;       /* [n_pods] new kai_pod_status */
    const int32_t* pod_node;         /* [n_pods] new node index (caller's order) or -1 */
    const int32_t* pod_gpu_group;    /* [n_pods] new shared-GPU group id or -1; NULL = unchanged */
    int32_t n_nodes;                 /* nodes whose state changed */
    const int32_t* node;             /* [n_nodes] node index (caller's order) */
    const uint32_t* node_flags;      /* [n_nodes] new KAI_NODE_* bits; NULL = unchanged */
    const double* node_allocatable;  /* [R][n_nodes] new status.allocatable; NULL = unchanged */
} kai_session_delta;
int kai_session_update(kai_core* core, const kai_session_delta* delta);

/* The cycle's clock (kai_config.now_ns; only the minruntime filters read it).  It takes effect at once on an open session, without any re-derivation, and is
 * what every later kai_session_open / kai_session_reset / kai_session_update of this handle uses.  Works without an open session. */
int kai_core_set_now(kai_core* core, int64_t now_ns);

/* What changes between two cycles beside the pods and nodes, none of it structural: the cycle's clock, queue rows (quota, limit, over-quota weight, the
 * normalised historical usage, priority, the two min-runtime settings) and the jobs' last start times.  Applied together with a pod / node delta by ONE pass:
 * one staging copy, one scatter, one re-derivation.
 *
 * Contract: the one of kai_session_update, extended.  Let S, cfg be the snapshot and the configuration of the last open or update and S', cfg' be them with
 * the delta and the rows applied.  After KAI_OK the handle is indistinguishable from a fresh handle created with cfg' that has run kai_session_open(S'):
 * read-backs bit for bit, everything every later action returns, and kai_session_reset returns to S'.
 *  - KAI_ERR_INVALID_ARG: what kai_session_update refuses in the delta; in the rows a wrong version, unknown `fields` bits, a negative count, a NULL index
 *    array with a count above 0, a queue or job index out of range or listed twice;
 *  - KAI_ERR_STATE: no open session;  KAI_ERR_UNSUPPORTED: a handle of a sharded group, and what kai_session_update refuses.
 *  Every refusal is decided before the first write, for both parts together: a valid delta with invalid rows writes nothing and leaves the session open on S.
 *  An optional array that was NULL at the open (queue_usage, job_last_start_ns, the two min-runtime arrays) exists in S' once a call carries it for at least
 *  one row, with the value an absent array stands for (0, 0, -1, -1) in every row the call does not name.
 *  delta and rows may each be NULL; kai_session_update(core, d) == kai_session_update_rows(core, d, NULL). */
#define KAI_ROWS_VERSION 1u
#define KAI_ROWS_HAS_NOW 0x1u
typedef struct kai_session_rows {
    uint32_t version;   /* KAI_ROWS_VERSION */
    uint32_t fields;    /* KAI_ROWS_HAS_NOW: now_ns is set */
    int64_t  now_ns;
    int32_t  n_queues;  /* queues whose rows changed */
    const int32_t* queue;                        /* [n_queues] queue index */
    const double*  queue_deserved;               /* [3][n_queues], units of the snapshot's; NULL = unchanged (likewise below) */
    const double*  queue_limit;                  /* [3][n_queues] */
    const double*  queue_oqw;                    /* [3][n_queues] */
    const double*  queue_usage;                  /* [3][n_queues] */
    const int32_t* queue_priority;               /* [n_queues] */
    const int64_t* queue_preempt_min_runtime_ns; /* [n_queues], -1 = not set on that queue */
    const int64_t* queue_reclaim_min_runtime_ns; /* [n_queues] */
    int32_t  n_jobs;    /* jobs whose rows changed */
    const int32_t* job;                          /* [n_jobs] job index */
    const int64_t* job_last_start_ns;            /* [n_jobs]; NULL = unchanged */
} kai_session_rows;
int kai_session_update_rows(kai_core* core, const kai_session_delta* delta, const kai_session_rows* rows);

/* replaces: ssn.QueueFairShare / QueueAllocatedResources / QueueDeservedResources
 * (plugins/proportion/proportion.go:508-521) */
int kai_queue_shares(kai_core* core, kai_queue_share* out, int cap);

/* replaces: Action.Execute(ssn) (actions/allocate/allocate.go:46-77, reclaim.go:47-100, preempt.go:46-97,
 * consolidation.go:32-78) up to, not including, the cache side effects of Statement.Commit
 * (framework/statement.go:536-575): the committed operations come back in commit order and the Go shim
 * replays them through cache.Bind / cache.Evict / cache.TaskPipelined. */
int kai_action_execute(kai_core* core, int action, kai_op* ops_out, int64_t ops_cap, int64_t* n_ops);

/* replaces: Session.OrderedNodesByTask + FittingNode for one task (framework/session.go:201-264),
 * against the session's current node state.  nodeset_bitmap (bit n of word n/32 = node index n, ceil(N/32) words) restricts the
 * node set as SubsetNodesFn would (framework/session_plugins.go:345-366); NULL = all nodes.  node_idx_out = -1 when nothing fits. */
int kai_best_node(kai_core* core, int32_t pod_idx, const uint32_t* nodeset_bitmap, int pipeline_only,
                  int32_t* node_idx_out, int* is_pipeline_out);

/* kai_best_node for MANY tasks in one chip-wide pass: out[i] is exactly what
 * kai_best_node(core, queries[i].pod, row queries[i].nodeset of nodeset_bitmaps or NULL, queries[i].flags & KAI_QUERY_PIPELINE_ONLY, ...)
 * returns at the same session state — the same node (caller's index, -1 when nothing fits) and the same is_pipeline.  nodeset is a row of
 * nodeset_bitmaps (n_nodesets rows of ceil(N/32) words, caller's node indices, the bit convention of kai_best_node) or -1 for all nodes; the
 * tasks of one job usually share a row.  The call changes nothing: read-backs, kai_action_stats_get and every later action are as if it had
 * not happened.  Like kai_best_node it does not look at the pod's status; duplicate queries are allowed.
 * n_queries == 0: KAI_OK without a launch.  KAI_ERR_INVALID_ARG: a NULL array with a count above 0, a negative count, a pod out of range,
 * a nodeset outside -1 .. n_nodesets-1, unknown flag bits, non-zero pad.  KAI_ERR_STATE: no open session.  KAI_ERR_UNSUPPORTED: a handle of
 * a sharded group (n_gpus > 1).  Every refusal is decided before the first device call and leaves out untouched.
 * On the device: one staging upload, three launches (k_bn_prep, k_bn_range, k_bn_scan; kai_best_nodes.hpp), one download and one stream
 * synchronise; the scratch belongs to the handle, grows on demand and is freed by kai_core_destroy. */
#define KAI_QUERY_PIPELINE_ONLY 0x1u
typedef struct kai_node_query  { int32_t pod; int32_t nodeset; uint32_t flags; int32_t pad; } kai_node_query;
typedef struct kai_node_answer { int32_t node; int32_t is_pipeline; } kai_node_answer;
int kai_best_nodes(kai_core* core, const kai_node_query* queries, int32_t n_queries,
                   const uint32_t* nodeset_bitmaps, int32_t n_nodesets, kai_node_answer* out);

/* The first k entries of the list kai_best_nodes answers the head of, for MANY tasks in one chip-wide pass.  For queries[i] take the node set of
 * kai_best_nodes (row queries[i].nodeset of nodeset_bitmaps, or all nodes for -1) and let L be Session.OrderedNodesByTask(nodeSet, task)
 * (framework/session.go:201-264: best score first, name rank on ties) with the nodes that fail FittingNode dropped, at the session's current state.
 * Then n_out[i] = min(k, |L|), out[i*k + j] for j < n_out[i] is the caller's index of L[j] with is_pipeline = PIPELINE_ONLY || !IsTaskAllocatable(task, L[j])
 * — the per-node rule kai_best_node applies to its one answer — and the entries j >= n_out[i] are {-1, 0}.  A task over its queue's capacity has n_out[i] = 0.
 * This is the list the reference's allocation walks (actions/common/allocate.go): a caller with a filter of its own (inter-pod affinity, host ports, volumes, DRA:
 * KAI_POD_CPU_FALLBACK pods) runs it down the list and stops at the first pass.  With k = 1 the call is kai_best_nodes, answer for answer.
 * The list is NOT "kai_best_node again with the winners removed from the node set": under a bin-pack strategy NodePreOrderFn
 * (plugins/nodeplacement/pack.go:66-86) takes the minimum and maximum of Idle + Releasing over the node set it is given, so removing a node can move them and
 * rescale every pack score against the other plugins' fixed scores.  Here the range is taken ONCE, over the whole node set, as the reference takes it.
 * The call changes nothing: read-backs, kai_action_stats_get and every later action are as if it had not happened.  It does not look at the pod's status;
 * duplicate queries are allowed.
 * n_queries == 0: KAI_OK without a launch.  KAI_ERR_INVALID_ARG: everything kai_best_nodes refuses, k < 1 or k > KAI_ORDERED_MAX_K, a NULL out or n_out with
 * n_queries > 0.  KAI_ERR_CAPACITY: n_queries * k above 2^27.  KAI_ERR_STATE: no open session.  KAI_ERR_UNSUPPORTED: a handle of a sharded group (n_gpus > 1).
 * Every refusal is decided before the first device call and leaves out and n_out untouched and the session open.
 * On the device: one staging upload, three launches (k_bn_prep, k_bn_range, k_on_scan; kai_ordered_nodes.hpp), one download and one stream synchronise; every
 * node is scored once per query, whatever k.  The scratch is kai_best_nodes': it belongs to the handle, grows on demand and is freed by kai_core_destroy. */
#define KAI_ORDERED_MAX_K 64
int kai_ordered_nodes(kai_core* core, const kai_node_query* queries, int32_t n_queries,
                      const uint32_t* nodeset_bitmaps, int32_t n_nodesets, int32_t k,
                      kai_node_answer* out /* [n_queries][k] */, int32_t* n_out /* [n_queries] */);

/* Committed operations taken back INTO the open session: what framework.Statement does with them (framework/statement.go), for operations an action of this
 * handle did not commit itself — an action the Go scheduler ran after a fallback, the operations of another handle (a standby scheduler, a what-if session).
 * The operations are taken in array order.  Each maximal run of equal `stmt` is one Statement: KAI_OP_ALLOCATE is Statement.Allocate(pod, node),
 * KAI_OP_PIPELINE is Statement.Pipeline(pod, node, updateTaskIfExistsOnNode = true), KAI_OP_EVICT is Statement.Evict(pod); the Statement is then
 * committed, so an allocated pod ends up Binding.
 *
 * Contract.  After KAI_OK the handle is indistinguishable from one whose own actions had committed exactly these operations: kai_pod_states,
 * kai_node_states and kai_queue_shares bit for bit, the same answers from kai_best_node(s), the same operations (kind, pod, node, job, stmt, seq) and
 * state from every later kai_action_execute.  kai_session_reset and kai_session_update* discard applied operations as they discard action results;
 * kai_action_stats_get is unaffected.
 * Fields: `node` is the caller's node index (for an evict: the node the pod is evicted from); `seq` and `job` are not read, so the array
 * kai_action_execute wrote can be passed as it is; `pad` must be 0; `stmt` must be non-decreasing.  Resource feasibility is not checked (Statement
 * does not check it either).
 * Per-operation precondition, against the state the preceding operations of the same call leave: ALLOCATE needs a Pending pod, PIPELINE a Pending or
 * Releasing pod, EVICT a pod that has a node, and op.node must be that node.
 * Every refusal is decided before the first write and leaves the session open and bit for bit unchanged; result->first_bad is the index of the first
 * offending operation, -1 on success and where no single operation is at fault (NULL ops, a negative count, unknown flags bits).
 *  - KAI_ERR_INVALID_ARG: NULL ops with n_ops > 0, a negative count, unknown flags bits, a kind outside 0..2, a pod or node index out of range, non-zero
 *    pad, a decreasing stmt;  KAI_ERR_CAPACITY: more than 2^31 - 16 operations;
 *  - KAI_ERR_STATE: no open session, or an operation whose precondition fails;
 *  - KAI_ERR_UNSUPPORTED: a handle of a sharded group (n_gpus > 1), or a session with shared-GPU requests (kai_op carries no GPU group).
 *  n_ops == 0: KAI_OK without a device call.
 * Two paths (kai_ops_apply.hpp), result->path says which one took the batch (with KAI_APPLY_CHECK_ONLY: which one would).  The chip-wide path takes a batch
 * that names every pod once, allocates / pipelines Pending pods and evicts Allocated, Binding, Bound or Running ones, in a session whose quantities add
 * exactly in any order (what the batch path of the allocate action asks for): one upload, two launches, one small download, one synchronise.  Everything
 * else — a pod evicted and pipelined again in one call — is walked by one lane through the engine's own Statement functions. */
#define KAI_APPLY_CHECK_ONLY  0x1u   /* validate, write nothing */
#define KAI_APPLY_ENGINE_PATH 0x2u   /* take the engine walk even where the chip-wide path qualifies (tests, A/B) */
#define KAI_APPLY_PATH_NONE 0
#define KAI_APPLY_PATH_WIDE 1
#define KAI_APPLY_PATH_ENGINE 2
typedef struct kai_apply_result { int64_t first_bad; int32_t path; int32_t statements; } kai_apply_result;
int kai_ops_apply(kai_core* core, const kai_op* ops, int64_t n_ops, uint32_t flags, kai_apply_result* result /* may be NULL */);

/* ONE open (uncommitted) Statement on the handle: framework.Statement as the allocate loop uses it (framework/statement.go:44-61, 522-575; allocateSubGroupSet
 * and attemptToAllocateJob in actions/common/allocate.go) — operations are applied WITHOUT the commit, logged on the device, rolled back to a checkpoint,
 * discarded or committed.  With the query calls (kai_ordered_nodes*, kai_subset_nodes*) it is the allocate loop for the jobs a caller places itself: try a node
 * set, roll back when the gang does not fit, try the next.
 *  - kai_stmt_begin opens the Statement (version: KAI_STMT_VERSION).  KAI_ERR_STATE with one open already.  Every other kai_stmt_* call without an open
 *    Statement: KAI_ERR_STATE.
 *  - kai_stmt_apply applies ops[0 .. n_ops) in array order and appends them to the log.  The fields of kai_op are read as kai_ops_apply reads them: `node` is the
 *    caller's index (for an evict: the node the pod is evicted from); `seq` and `job` are not read; `pad` must be 0; `stmt` is not read (there is one Statement).
 *    KAI_OP_ALLOCATE is Statement.Allocate: the pod is left ALLOCATED, not Binding.  KAI_OP_PIPELINE is Statement.Pipeline(updateTaskIfExistsOnNode = true).
 *    KAI_OP_EVICT is Statement.Evict and needs a pod on op.node.  The per-operation preconditions are kai_ops_apply's, against the state the Statement has
 *    reached.  A failing precondition: KAI_ERR_STATE, result->first_bad is the operation, nothing is written, the Statement stays open with its log as it was.
 *    The log has room for n_pods * 2 + 32 operations (half of the device log: the engine's rollback pushes one undo record per undone operation on top of the
 *    log before it truncates, so a discard of L records needs 2 L of them); a call that would exceed it: KAI_ERR_CAPACITY, nothing is written.
 *    KAI_APPLY_CHECK_ONLY validates and writes nothing.  n_ops == 0: KAI_OK without a device call.
 *  - kai_stmt_checkpoint: *cp_out = the log's length.  Host only: no device call.
 *  - kai_stmt_rollback(cp) undoes the operations [cp, log_len), last first as Statement.Rollback does.  Afterwards the handle is indistinguishable from a twin on
 *    which kai_stmt_begin and only the first cp operations were applied: kai_pod_states, kai_node_states and kai_queue_shares bit for bit, the answers of
 *    kai_best_node(s), kai_ordered_nodes*, kai_subset_nodes* and kai_job_order, and everything after a later commit — the operations and kai_action_stats of
 *    the next actions included (rolled-back evictions and pipelines do not keep the allocate action off its batch path).  cp outside 0 .. log_len:
 *    KAI_ERR_INVALID_ARG.  cp == log_len: KAI_OK without a launch.
 *  - kai_stmt_discard is kai_stmt_rollback(0), then the Statement is closed.  In a session whose quantities add exactly (whole GPUs, integral milli-CPU and
 *    memory: what the batch path of the allocate action asks for) the three read-backs afterwards equal those before kai_stmt_begin bit for bit.
 *  - kai_stmt_commit commits as Statement.Commit does (an allocated pod becomes Binding) and closes the Statement.  Afterwards the handle is indistinguishable
 *    from one on which kai_ops_apply took the surviving operations as one Statement.  ops_out (may be NULL) gets them as kai_op: seq from 0, stmt 0, job filled,
 *    nodes in the caller's indices; *n_ops (may be NULL) their number.  ops_cap below it: KAI_ERR_CAPACITY with *n_ops set, the Statement stays open and
 *    uncommitted.
 * While a Statement is open: every query call and the three read-backs work, see the tentative state and leave the log untouched.  kai_action_execute,
 * kai_ops_apply and kai_stale_gang_eviction return KAI_ERR_STATE and write nothing.  kai_session_open, kai_session_reset, kai_session_update* and
 * kai_session_close drop the Statement with everything else they drop.
 * Other refusals, as kai_ops_apply's: KAI_ERR_UNSUPPORTED for a handle of a sharded group (n_gpus > 1) and for a session with shared-GPU requests;
 * KAI_ERR_INVALID_ARG for a wrong version, NULL ops with n_ops > 0, a negative count, unknown flags bits (kai_stmt_apply: KAI_APPLY_CHECK_ONLY,
 * KAI_APPLY_ENGINE_PATH; rollback and discard: KAI_APPLY_ENGINE_PATH), a kind outside 0..2, a pod or node index out of range, non-zero pad, a NULL cp_out, a
 * negative ops_cap or NULL ops_out with ops_cap > 0.  Every refusal is decided before the first write.  KAI_ERR_DEVICE_FAULT (the engine's own state disagrees
 * with the pod states) and any other failure behind the first launch (KAI_ERR_HIP, KAI_ERR_NO_MEMORY) close the Statement; kai_session_reset is the way on.
 * result (may be NULL): first_bad as in kai_apply_result; log_len the log's length after the call (0 after discard and commit); path (KAI_APPLY_PATH_*) the
 * path that took the call.  Two paths over one log (kai_stmt.hpp; the engine's own Statement records, so either path takes over at any point): chip-wide
 * kernels where every pod is named at most once in the surviving log plus the batch and every operation starts from a state kai_ops_apply's chip-wide path
 * takes — apply: one upload, two launches; rollback, discard, commit: one launch; each one small download and one synchronise — and one lane through the
 * engine's own Statement functions for everything else (KAI_APPLY_ENGINE_PATH: also where the chip-wide path qualifies).
 * Not covered: Pipeline with updateTaskIfExistsOnNode = false and Statement.Unevict; ConvertAllAllocatedToPipelined (roll back and pipeline instead); several
 * open Statements. */
#define KAI_STMT_VERSION 1u
typedef struct kai_stmt_result { int64_t first_bad; int64_t log_len; int32_t path; int32_t pad; } kai_stmt_result;
int kai_stmt_begin(kai_core* core, uint32_t version);
int kai_stmt_apply(kai_core* core, const kai_op* ops, int64_t n_ops, uint32_t flags, kai_stmt_result* result /* may be NULL */);
int kai_stmt_checkpoint(kai_core* core, int64_t* cp_out);
int kai_stmt_rollback(kai_core* core, int64_t cp, uint32_t flags, kai_stmt_result* result /* may be NULL */);
int kai_stmt_discard(kai_core* core, uint32_t flags, kai_stmt_result* result /* may be NULL */);
int kai_stmt_commit(kai_core* core, kai_op* ops_out /* may be NULL */, int64_t ops_cap, int64_t* n_ops /* may be NULL */, kai_stmt_result* result /* may be NULL */);

/* replaces: the stalegangeviction action (actions/stalegangeviction/stalegangeviction.go:29-90), the fifth of the default action list.  The decision is taken on
 * the device against the session's CURRENT state (after whatever actions or kai_ops_apply calls ran) and the evictions are applied as kai_ops_apply applies
 * KAI_OP_EVICT operations (ssn.Evict, framework/session.go:127-150).
 * A job is stale (PodGroupInfo.IsStale, api/podgroup_info/job_info.go:417-432) when none of its pods is Succeeded, at least one is active-used (Allocated,
 * Pipelined, Binding, Bound, Running, Releasing) and some pod-set has fewer active-used pods than its minAvailable.  The clock is the handle's
 * (kai_core_set_now); it must be above 0, because 0 stands for "no timestamp" in job_stale_since_ns.
 *  - job_stale_since_ns [n_jobs], in/out: StalenessInfo.TimeStamp, 0 = nil.  Afterwards: 0 for a job that is not stale, unchanged for a job that was stale
 *    already, now for a newly stale job — also with a negative grace period (the reference stamps before it looks at the period).
 *  - a stale job is evicted when now - since >= grace_ns (grace_ns < 0: never): job_stale_out[j] (may be NULL) is 1 exactly for those jobs (StalenessInfo.Stale),
 *    also where no pod is left to evict (a job whose active pods are all Releasing); result->stale_jobs counts the stale jobs, result->expired_jobs the evicted.
 *  - ops_out: one KAI_OP_EVICT per pod of an evicted job with an active-allocated status (the set above without Releasing), in ascending pod index (the
 *    reference walks Go maps and fixes no order; this is the library's).  node: the caller's index of the pod's node; job: the pod's job; seq counts from 0;
 *    stmt is one number per job, from 0 in array order — a job's pods are contiguous, so the length of its run of equal stmt is its EvictionGangSize; pad 0.
 *    The array can be passed to kai_ops_apply of another handle as it is.
 * After KAI_OK without KAI_STALE_DRY_RUN the handle is indistinguishable from a twin in the same state on which kai_ops_apply(ops_out, *n_ops) ran:
 * kai_pod_states, kai_node_states and kai_queue_shares bit for bit, the answers of kai_best_node(s), every later action.  kai_session_reset and
 * kai_session_update* discard the evictions as they discard action results; kai_action_stats_get is unaffected.  With KAI_STALE_DRY_RUN the session stays
 * bit for bit as it was and everything is reported the same way; result->path (KAI_APPLY_PATH_*) then says which apply path would run.  Nothing to evict:
 * KAI_OK, *n_ops = 0, the timestamps are updated, no apply launch.
 * Refusals, all decided before the first write to the session and to the caller's arrays:
 *  - KAI_ERR_INVALID_ARG: a wrong version, unknown flag bits, NULL params / job_stale_since_ns / n_ops, NULL ops_out with ops_cap > 0, a negative capacity,
 *    a negative job_stale_since_ns entry, a clock that is not above 0;
 *  - KAI_ERR_STATE: no open session;
 *  - KAI_ERR_UNSUPPORTED: a handle of a sharded group (n_gpus > 1); a session with shared-GPU requests — kai_ops_apply's restriction (kai_op carries no GPU
 *    group), not lifted here;
 *  - KAI_ERR_CAPACITY: ops_cap is below the number of evictions; *n_ops holds the number needed (n_pods always suffices). */
#define KAI_STALE_VERSION 1u
#define KAI_STALE_DRY_RUN 0x1u   /* decide and report; the session is not written */
typedef struct kai_stale_params { uint32_t version; uint32_t flags; int64_t grace_ns; /* < 0: never evict */ } kai_stale_params;
typedef struct kai_stale_result { int32_t stale_jobs; int32_t expired_jobs; int64_t n_ops; int32_t path; int32_t pad; } kai_stale_result;
int kai_stale_gang_eviction(kai_core* core, const kai_stale_params* params,
                            int64_t* job_stale_since_ns /* [n_jobs] in/out, 0 = nil */, uint8_t* job_stale_out /* [n_jobs] or NULL: StalenessInfo.Stale */,
                            kai_op* ops_out, int64_t ops_cap, int64_t* n_ops, kai_stale_result* result /* may be NULL */);

/* replaces: the reflectjoborder plugin's computation (plugins/reflectjoborder/reflect_job_order.go:41-66, served as /get-job-order): in what order are the
 * queued jobs served, and where does a job stand in its queue?
 *  - order_out[0 .. *n_out) is the sequence of PopNextJob results (actions/utils/job_order_by_queue.go:61-89) of a JobsOrderByQueues built with FilterNonPending,
 *    FilterUnready (actions/utils/input_jobs.go:21-68), the given depth and VictimQueue = false over all jobs, at the session's CURRENT state: after whatever
 *    actions, kai_ops_apply or kai_stale_gang_eviction calls ran — shares, pod statuses and elastic state as they are now.  Nothing is allocated between pops.
 *    params->depth: 0 = kai_config.queue_depth[KAI_ACTION_ALLOCATE] (what reflectjoborder takes, ssn.GetJobsDepth), -1 = infinite, > 0 = that many jobs per leaf queue.
 *  - job_pos_out[j] (may be NULL) is job j's position in that sequence (GlobalOrder); job_queue_pos_out[j] (may be NULL) its position among the jobs of its own
 *    leaf queue, QueueOrder[job.Queue] of the reference (:61-62): what a "position in queue" display shows.  Both are -1 for a job that is not in the order.
 *  - result (may be NULL): n_ordered = *n_out; path (KAI_JOB_ORDER_PATH_*) = what ordered; n_leaves = leaf queues with a job in the order (the keys of QueueOrder).
 * The call changes nothing: kai_pod_states, kai_node_states, kai_queue_shares, kai_action_stats_get, the answers of kai_best_node(s) / kai_ordered_nodes and every
 * later action, kai_ops_apply or kai_session_update* are as if it had not happened.  It re-derives what every action's own init re-derives before anything reads
 * it: the jobs' filter / elastic state (j_state), the tasks-to-allocate chunks where their cache is invalid (job_info.go:253-256 invalidates it with every status
 * change; the chunk is a function of the current state), the leaves' sorted regions and side heaps and the records and heaps of the job-order tree.  Nothing
 * reads those between actions: kai_action_execute rebuilds them (k_job_init, k_leaf_init, Engine::init_jobs_order) before its first pop.
 * Two paths, the same order.  Chip-wide (KAI_JOB_ORDER_PATH_WIDE): no pop changes any share, so the order is one bottom-up pass of scans and merges over the queue
 * tree, the allocate action's plan with constant shares — taken when the siblings' static order (queue_order.go:214-240) is strict in every sibling set, the tree has
 * at most 16 levels, the proportion plugin orders the queues and every queued job is below minAvailable with a valid tasks-to-allocate chunk; the jobs need not be
 * plain gangs and a finite depth does not disqualify.  Otherwise (KAI_JOB_ORDER_PATH_ENGINE) one lane walks the engine's own job-order tree until it is empty.
 * A session with shared-GPU requests is not refused: nothing is allocated.  No queued job: KAI_OK, *n_out = 0, path KAI_JOB_ORDER_PATH_NONE.
 * Refusals, all decided before the first device call, leave every output untouched:
 *  - KAI_ERR_INVALID_ARG: a wrong version, unknown flag bits, non-zero pad, depth < -1, NULL params / n_out, NULL order_out with cap > 0, a negative cap;
 *  - KAI_ERR_STATE: no open session;  KAI_ERR_UNSUPPORTED: a handle of a sharded group (n_gpus > 1).
 * KAI_ERR_CAPACITY: cap is below the number of ordered jobs, known once the device has counted them; *n_out holds the number needed (n_jobs always suffices), the
 * other outputs are untouched. */
#define KAI_JOB_ORDER_VERSION 1u
#define KAI_JOB_ORDER_ENGINE_PATH 0x1u   /* take the heap walk even where the chip-wide path qualifies (tests, A/B) */
#define KAI_JOB_ORDER_PATH_NONE 0
#define KAI_JOB_ORDER_PATH_WIDE 1
#define KAI_JOB_ORDER_PATH_ENGINE 2
typedef struct kai_job_order_params { uint32_t version; uint32_t flags; int32_t depth; int32_t pad; } kai_job_order_params;
typedef struct kai_job_order_result { int32_t n_ordered; int32_t path; int32_t n_leaves; int32_t pad; } kai_job_order_result;
int kai_job_order(kai_core* core, const kai_job_order_params* params,
                  int32_t* order_out, int32_t cap, int32_t* n_out,          /* job indices in pop order */
                  int32_t* job_pos_out /* [n_jobs] or NULL */, int32_t* job_queue_pos_out /* [n_jobs] or NULL */,
                  kai_job_order_result* result /* may be NULL */);

/* replaces: the SubsetNodesFn of the default tier, the topology plugin's subSetNodesFn (plugins/topology/job_filtering.go:34-112), for MANY jobs, sub-groups or
 * pod-sets at once: which node sets does the allocate action walk for this gang, and in which order?  The answer comes as bitmap rows that go into
 * kai_best_nodes / kai_ordered_nodes as nodeset_bitmaps rows unchanged.
 *  - queries[i] asks what subSetNodesFn(job, subGroup, podSets, tasks, nodeSet) returns at the session's CURRENT state (after whatever actions, kai_ops_apply or
 *    kai_stale_gang_eviction calls ran).  subGroup: group == -1 and podset == -1: the job's root sub-group set; group >= 0: that SubGroupSet (a group of `job`;
 *    podset must be -1); podset >= 0: that pod-set with its own constraint (a pod-set of `job`; group must be -1).  A snapshot without groups has the root form only.
 *    tasks: the job's GetTasksToAllocate chunk with isRealAllocation = true at the current state, restricted to the sub-group (what the allocate action hands
 *    over).  nodeSet: row `nodeset` of nodeset_bitmaps (the rows and bit convention of kai_best_nodes), -1 = all nodes.
 *  - answers_out[i]: status (KAI_SUBSET_*); n_sets; first = where the query's n_sets records start in sets_out (records lie in query order: the running sum of
 *    n_sets); tasks = len(tasks); common_domain = what lowestCommonDomainID chose, in kai_node_set.domain's encoding, KAI_SUBSET_PARENT where the function
 *    returned before it.
 *  - sets_out[first + k]: the k-th node set the action tries (sortDomainInfos: deepest level first, tree order inside a level after sortTreeFromRoot).  domain: the
 *    caller's index into the snapshot's domain table, KAI_SUBSET_ROOT(t) for the root domain of topology t, or KAI_SUBSET_PARENT = "the parent node set as it
 *    is"; level: the level inside the topology, -1 for a root and for PARENT; allocatable_pods: the domain's AllocatablePods, -1 where representor accounting was
 *    not used (useRepresentorPodsAccounting false) and for PARENT; n_nodes: the size of the set.
 *  - bitmaps_out (may be NULL), row first + k: the set's nodes — the domain's nodes that are in the parent set (all of them part of the topology: the valid nodes
 *    of lowestCommonDomainID) — in the caller's node indices.
 * The reference's order of decisions is the contract (job_filtering.go:38-111): a topology that does not exist (constraint topology -2): KAI_SUBSET_NO_TOPOLOGY;
 * no constraint, no topology plugin or no task: one set, KAI_SUBSET_PARENT; a common domain that cannot take the tasks: KAI_SUBSET_NO_FIT (before the level check:
 * a bad level on a gang that does not fit anyway is NO_FIT); no level given, or a level the topology does not have: KAI_SUBSET_BAD_LEVEL (the function returns an
 * error); no fitting domain on the relevant levels: KAI_SUBSET_NO_FIT; otherwise the ordered list — restricted to the sub-trees that already hold an active pod
 * of the sub-group where a required level is set (getRelevantDomainsWithAllocatedPods).
 * The call changes nothing: kai_pod_states, kai_node_states, kai_queue_shares, kai_action_stats_get, the answers of kai_best_node(s) / kai_ordered_nodes /
 * kai_job_order and every later action, kai_ops_apply or kai_session_update* are as if it had not happened.  It re-derives what every action's own init
 * re-derives before anything reads it: the tasks-to-allocate chunks of the queried jobs where their cache is invalid, and — on the engine path — the scratch
 * tables of the domain tree (free resources, allocatable pods, ratios, keys), the order of the children inside a sibling set (every subSetNodesFn of an action
 * sorts the sets it reads first) and the slots of the preferred-level node scores.  The scores themselves (calculateNodeScores) are returned by kai_subset_nodes_scored
 * (below) and taken by kai_ordered_nodes_scored; this call returns none, and kai_best_nodes / kai_ordered_nodes score without a topology term.
 * Two paths, the same answer.  Chip-wide (KAI_SUBSET_PATH_WIDE): a workgroup per query surveys the nodes, rolls the sums up the tree in a table of its own, ranks
 * the siblings and lists the fitting domains; taken for the whole call when the topology plugin is loaded, the session's quantities add exactly in any order,
 * there are no shared-GPU requests and no MIG rows, and every topology has at most 8 levels and paths that fit 63 bits ((domains + topologies)^levels).
 * Otherwise, and with KAI_SUBSET_ENGINE_PATH, one lane calls the engine's own subset_nodes query by query (KAI_SUBSET_PATH_ENGINE).  Sibling sets that
 * sortTreeFromRoot does not reach (outside the common domain's sub-tree, or below the preferred level where the required level lies deeper) have no order in the
 * reference; the chip-wide path lists them by domain index, the engine path as the last action left them.
 * Refusals, all decided before the first write to any output, leave the session open and unchanged:
 *  - KAI_ERR_INVALID_ARG: a wrong version, unknown flag bits; a negative count or capacity; a NULL array with a count above 0, NULL params or
 *    n_sets_out; a job, group, pod-set or nodeset out of range; a group or pod-set that is not the job's; both group and podset given;
 *  - KAI_ERR_STATE: no open session;  KAI_ERR_UNSUPPORTED: a handle of a sharded group (n_gpus > 1).
 * KAI_ERR_CAPACITY: the sets of all queries exceed sets_cap, known once the device has counted them; *n_sets_out holds the number needed and the other outputs
 * are untouched.  n_queries x (domains of the largest topology + 1) always suffices.  n_queries == 0: KAI_OK without a launch, *n_sets_out = 0, path NONE. */
#define KAI_SUBSET_VERSION 1u
#define KAI_SUBSET_ENGINE_PATH 0x1u      /* take the engine walk even where the chip-wide path qualifies (tests, A/B) */
#define KAI_SUBSET_PATH_NONE 0
#define KAI_SUBSET_PATH_WIDE 1
#define KAI_SUBSET_PATH_ENGINE 2
#define KAI_SUBSET_PARENT (-1)           /* kai_node_set.domain: "the parent node set as it is" */
#define KAI_SUBSET_ROOT(t) (-2 - (t))    /* the root domain of topology t: every node of the parent set that is part of t */
enum { KAI_SUBSET_OK = 0,          /* n_sets >= 1 */
       KAI_SUBSET_NO_TOPOLOGY = 1, /* the named topology does not exist (constraint topology -2): no set */
       KAI_SUBSET_NO_FIT = 2,      /* the common domain, or every domain of the relevant levels, cannot take the tasks: no set */
       KAI_SUBSET_BAD_LEVEL = 3 }; /* the function returns an error: no level given, or a level the topology does not have */
typedef struct kai_subset_params { uint32_t version; uint32_t flags; } kai_subset_params;
typedef struct kai_subset_query  { int32_t job; int32_t group; int32_t podset; int32_t nodeset; } kai_subset_query;
typedef struct kai_subset_answer { int32_t status; int32_t n_sets; int32_t first; int32_t tasks; int32_t common_domain; int32_t pad; } kai_subset_answer;
typedef struct kai_node_set      { int32_t domain; int32_t level; int32_t allocatable_pods; int32_t n_nodes; } kai_node_set;
typedef struct kai_subset_result { int64_t n_sets; int32_t path; int32_t pad; } kai_subset_result;
int kai_subset_nodes(kai_core* core, const kai_subset_params* params,
                     const kai_subset_query* queries, int32_t n_queries,
                     const uint32_t* nodeset_bitmaps, int32_t n_nodesets,      /* parent node sets: the rows and bit convention of kai_best_nodes */
                     kai_subset_answer* answers_out /* [n_queries] */,
                     kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out,
                     uint32_t* bitmaps_out /* [sets_cap][ceil(N/32)] or NULL */,
                     kai_subset_result* result /* may be NULL */);

/* kai_subset_nodes with the topology plugin's node scores: what t.subGroupNodeScores[subGroup] holds when subSetNodesFn returns (plugins/topology/job_filtering.go:87-90,
 * calculateNodeScores, node_scoring.go:37-53).  Every output of kai_subset_nodes comes back byte for byte as that call returns it for the same arguments: the same two
 * paths with the same qualification, KAI_SUBSET_ENGINE_PATH, the same refusals in the same precedence; the call changes nothing in the session either.  Per query it adds
 *  - score_rows_out[i].level_row: the row of the snapshot's node_domain a node's domain is read from, topo_level_off[t] + preferredLevel, where scores were recorded:
 *    exactly when the function gets past checkJobDomainFit on the common domain with a preferred level set — decided in front of the level checks, so a query that ends
 *    KAI_SUBSET_BAD_LEVEL because of its required level, or KAI_SUBSET_NO_FIT on the relevant levels, still has scores.  n_scored: the preferred-level domains in the
 *    common domain's sub-tree.
 *  - deciles_out[i * n_domains + d] = floor((idx + 1) / n_scored * 10) (0 .. 10, the reference's arithmetic in double) for such a domain d, in the caller's domain
 *    indices, at place idx of getLevelDomains' depth-first order over the children as sortTreeFromRoot left them (ratio descending, domain_id_rank ascending);
 *    KAI_TOPO_NO_SCORE for every other domain.  A node's score is decile x KAI_TOPO_SCORE_UNIT: decile 0 is a score (0.0), 255 is none.  A common domain that is itself
 *    at the preferred level: one domain, decile 10.
 *  - {KAI_TOPO_SCORES_NONE, 0} and a row of 255 where the function records nothing: no topology plugin, no constraint, topology -2, no task, a common domain that does not
 *    fit, no preferred level.  The reference then looks at the sub-group's ancestors (getRelevantNodeScores, node_scoring.go:88-99).  WHICH ROW A TASK USES IS THE
 *    CALLER'S CHOICE: its pod-set's row, else the nearest ancestor group's that is not NONE; scores are computed once per sub-group and not again between the tasks of a gang.
 *  - {KAI_TOPO_SCORES_EMPTY, 0} and a row of 255 for a preferred level the topology does not have: the reference stores an empty map and every node fails the lookup.
 * Additional refusal: NULL score_rows_out or deciles_out with n_queries > 0 is KAI_ERR_INVALID_ARG.  On KAI_ERR_CAPACITY the two outputs stay untouched, like the others. */
#define KAI_TOPO_SCORE_UNIT   10000.0   /* scores.Topology */
#define KAI_TOPO_NO_SCORE     255       /* decile of a domain whose nodes have no score: such a node is dropped from the list */
#define KAI_TOPO_SCORES_NONE  (-1)      /* level_row: the call left no scores for this sub-group (term 0, no node dropped) */
#define KAI_TOPO_SCORES_EMPTY (-2)      /* level_row: scores were recorded but the preferred level is none of the topology's: every node is dropped */
typedef struct kai_topo_score_row { int32_t level_row; int32_t n_scored; } kai_topo_score_row;
int kai_subset_nodes_scored(kai_core* core, const kai_subset_params* params,
                            const kai_subset_query* queries, int32_t n_queries,
                            const uint32_t* nodeset_bitmaps, int32_t n_nodesets,
                            kai_subset_answer* answers_out /* [n_queries] */,
                            kai_node_set* sets_out, int64_t sets_cap, int64_t* n_sets_out,
                            uint32_t* bitmaps_out /* [sets_cap][ceil(N/32)] or NULL */,
                            kai_topo_score_row* score_rows_out /* [n_queries] */, uint8_t* deciles_out /* [n_queries][n_domains] */,
                            kai_subset_result* result /* may be NULL */);

/* kai_ordered_nodes with the topology plugin's term (nodeOrderFn, plugins/topology/node_scoring.go:17-35).  queries[i].scores names a row of score_rows / deciles
 * (n_score_rows rows, deciles [n_score_rows][n_domains], as kai_subset_nodes_scored wrote them), -1 = none.  With scores = s >= 0 and score_rows[s].level_row >= 0,
 * node n of the node set has the domain dd = node_domain[level_row][n]: with dd < 0 or deciles[s][dd] == KAI_TOPO_NO_SCORE the node is dropped from the list (a node
 * without a score raises an error in the reference and OrderedNodesByTask drops it, framework/session.go:247-251); otherwise its score is kai_ordered_nodes' score plus
 * deciles[s][dd] x KAI_TOPO_SCORE_UNIT — the rule the allocate action applies on the device.  level_row == KAI_TOPO_SCORES_EMPTY: n_out[i] = 0.  scores = -1, a
 * KAI_TOPO_SCORES_NONE row, or a configuration without KAI_PLUGIN_TOPOLOGY: the query is answered exactly as kai_ordered_nodes answers it.
 * Everything else is kai_ordered_nodes': the bin-pack pre-order range is taken once over the WHOLE node set, dropped nodes included (NodePreOrderFn runs before any
 * score); is_pipeline; n_out and the {-1, 0} tail; k = 1 .. KAI_ORDERED_MAX_K (k = 1 is "kai_best_nodes_scored"); duplicates allowed; no look at the pod's status;
 * sessions with shared GPUs / MIG are served; one staging upload (the score rows and deciles ride in it), three launches, one download, one synchronise.
 * Refusals, decided before the first device call, outputs untouched: everything kai_ordered_nodes refuses (there is no pad field); scores outside -1 .. n_score_rows-1;
 * a negative n_score_rows; NULL score_rows / deciles with n_score_rows > 0; a level_row outside -2 .. n_topo_levels-1; a decile that is neither <= 10 nor 255.
 * n_queries == 0: KAI_OK without a launch. */
typedef struct kai_scored_query { int32_t pod; int32_t nodeset; uint32_t flags; int32_t scores; } kai_scored_query;  /* scores: row of score_rows / deciles, -1 = none */
int kai_ordered_nodes_scored(kai_core* core, const kai_scored_query* queries, int32_t n_queries,
                             const uint32_t* nodeset_bitmaps, int32_t n_nodesets,
                             const kai_topo_score_row* score_rows, const uint8_t* deciles, int32_t n_score_rows,
                             int32_t k, kai_node_answer* out /* [n_queries][k] */, int32_t* n_out /* [n_queries] */);

/* replaces: the innermost part of the allocate loop (actions/common/allocate.go:83-107 allocatePodSet with allocateTasksOnNodeSet inside) for gangs a caller places
 * itself: per gang the loop over its node sets, per set the chain of its tasks' placements, inside the open Statement and over the Statement's own log — ONE call for
 * many gangs instead of two calls (kai_ordered_nodes with k = 1, kai_stmt_apply of one operation) per task.  The sets come from kai_subset_nodes(_scored); the call is
 * allocatePodSet without its SubsetNodesFn.  It is indistinguishable from this loop over the existing calls, on the same handle in the same state:
 *
 *   for g in gangs, in array order:
 *       cp = kai_stmt_checkpoint()
 *       for s in sets[g.first_set .. g.first_set + g.n_sets), in order:
 *           for t in tasks[g.first_task .. g.first_task + g.n_tasks), in order:
 *               a = kai_ordered_nodes_scored(k = 1, {pod t, nodeset s, flags & KAI_PLACE_PIPELINE_ONLY, scores g.scores})     at the state reached
 *               if a is empty: fail_at[s] = index of t in the gang; kai_stmt_rollback(cp); try the next set
 *               kai_stmt_apply({a.is_pipeline ? KAI_OP_PIPELINE : KAI_OP_ALLOCATE, t, a.node})
 *           if every task was placed: fail_at[s] = n_tasks; status KAI_PLACE_PLACED, set = position of s in the gang's list; go to the next gang
 *       status KAI_PLACE_NO_FIT: its operations are gone, the gangs before it keep theirs, the next gang goes on
 *
 * — kai_pod_states, kai_node_states and kai_queue_shares bit for bit, the answers of every query call, the log, and everything a later kai_stmt_rollback (on either of
 * its paths, to any checkpoint, the caller's earlier ones included), discard, commit or action gives.  The Statement stays open; only the call's own operations are
 * rolled back, so a caller's outer checkpoint (a sub-group tree) still works.
 * Outputs: answers_out[g]: status, set (-1: none), sets_tried, and first_op / n_ops: the gang's surviving operations in ops_out.  fail_at_out (may be NULL) is indexed
 * like `sets`: the gang index of the first task the set had no node for (handleFailedTaskAllocation's numSchedulableTasks), n_tasks for the set that took the gang, -1
 * for an entry that was not tried.  ops_out: the call's surviving operations in log order — kind, pod, node (the caller's index), job, seq = the position in the log,
 * stmt 0; *n_ops (may be NULL) their number.  result (may be NULL): log_len after the call; path: KAI_APPLY_PATH_WIDE where the session qualifies for the chip-wide
 * kernels (the records are then undone and committed by them), KAI_APPLY_PATH_ENGINE where the placing lane went through the engine's own Statement functions
 * (KAI_APPLY_ENGINE_PATH: also where the chip-wide path qualifies).  The node search is the same in both.
 * Refusals, all decided before the first write; the Statement stays open with its log as it was:
 *  - what every kai_stmt_* call refuses (no session, no open Statement: KAI_ERR_STATE; a sharded handle, shared-GPU requests: KAI_ERR_UNSUPPORTED);
 *  - KAI_ERR_INVALID_ARG: a wrong version, unknown flags, non-zero pad, a negative count, a NULL array with a count above 0, a gang's range outside tasks / sets, a gang
 *    with n_tasks < 1 or n_sets < 1, a pod, set row or score row out of range, what kai_ordered_nodes_scored refuses in score rows and deciles, a pod named twice in tasks, an entry of tasks that two gangs share;
 *  - KAI_ERR_STATE with result->first_bad = the index in `tasks` of the first pod that is not Pending at entry (decided by the first launch);
 *  - KAI_ERR_CAPACITY: the log's length plus n_tasks above its room (2 n_pods + 32), ops_cap below n_tasks, or the sum of n_tasks x n_sets over the gangs above 2^20
 *    (one workgroup walks the chain: its running time is bounded by that sum times the size of a set).
 * n_gangs == 0: KAI_OK without a device call.  Of nodeset_bitmaps only the rows that `sets` names are read and uploaded.  One staging upload, two launches (k_sp_prep chip-wide: the Pending check, every named set row compacted into an
 * ascending name-rank list, so that a task's scan costs the set's size and not n_nodes; k_sp_place: one workgroup), one download, one synchronise. */
#define KAI_PLACE_VERSION 1u
#define KAI_PLACE_PIPELINE_ONLY 0x4u       /* isPipelineOnly for every task of the call; beside KAI_APPLY_ENGINE_PATH */
enum { KAI_PLACE_PLACED = 0, KAI_PLACE_NO_FIT = 1 };
typedef struct kai_place_params { uint32_t version; uint32_t flags; } kai_place_params;
typedef struct kai_place_gang   { int32_t first_task, n_tasks;   /* tasks[first_task ..): pod indices, in the order they are placed */
                                  int32_t first_set,  n_sets;    /* sets[first_set ..): rows of nodeset_bitmaps in the order they are tried, -1 = all nodes */
                                  int32_t scores;                /* row of score_rows / deciles (kai_ordered_nodes_scored), -1 = none */
                                  int32_t pad; } kai_place_gang;
typedef struct kai_place_answer { int32_t status; int32_t set;   /* index in the gang's own list of the set that took it, -1 */
                                  int32_t sets_tried; int32_t pad;
                                  int64_t first_op; int64_t n_ops; /* its surviving operations in ops_out */ } kai_place_answer;
int kai_stmt_place(kai_core* core, const kai_place_params* params,
                   const kai_place_gang* gangs, int32_t n_gangs,
                   const int32_t* tasks, int32_t n_tasks, const int32_t* sets, int32_t n_sets,
                   const uint32_t* nodeset_bitmaps, int32_t n_nodesets,
                   const kai_topo_score_row* score_rows, const uint8_t* deciles, int32_t n_score_rows,
                   kai_place_answer* answers_out /* [n_gangs] */,
                   int32_t* fail_at_out /* [n_sets] or NULL */,
                   kai_op* ops_out, int64_t ops_cap, int64_t* n_ops /* may be NULL */,
                   kai_stmt_result* result /* may be NULL */);

/* session-state read-back (what the shim mirrors into PodInfo.Status/NodeName and NodeInfo.Idle/Releasing) */
int kai_pod_states(kai_core* core, int32_t* status_out, int32_t* node_out, int cap);
int kai_node_states(kai_core* core, kai_node_state* out, int cap);

/* PodInfo.GPUGroups[0] of every active fraction pod after the actions run so far (what a BindRequest carries as SelectedGPUGroups,
 * cache/cache.go:290-330): the snapshot's group id, or an id >= 2^20 for a group the cycle opened (gpu_sharing/gpuSharing.go:73-83); -1 otherwise */
int kai_pod_gpu_groups(kai_core* core, int32_t* groups_out, int cap);

int kai_action_stats_get(kai_core* core, kai_action_stats* out);

/* replaces: framework.CloseSession (framework/framework.go:67-78) — frees the session's HBM */
int kai_session_close(kai_core* core);

/* human-readable detail for the last non-zero status on this handle (never NULL) */
const char* kai_last_error(kai_core* core);

/* library build info: "kai_core <abi> gfx950 …" */
const char* kai_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KAI_CORE_H */
