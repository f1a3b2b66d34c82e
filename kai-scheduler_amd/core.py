"""Host-side mirror of the reference's Session / Action interface over the C ABI (libkai_core.so).

    core = KaiCore(cfg)                       # scheduler.NewScheduler  (pkg/scheduler/scheduler.go:53-101)
    ssn  = core.open_session(snapshot)        # framework.OpenSession   (framework/framework.go:32-65)
    ops  = ssn.execute("allocate")            # Action.Execute(ssn)     (actions/allocate/allocate.go:46-77)
    ssn.queue_shares(); ssn.pod_states()      # what the Go shim mirrors back into the Session
    ssn.close()                               # framework.CloseSession

The library is the only implementation: if it (or a HIP device) is missing this module raises — there is
no Python or CPU fallback of the path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KAI_CORE_LIB") or os.path.join(_HERE, "csrc", "libkai_core.so")  # KAI_CORE_LIB: another BUILD of the same HIP library (profiling variants)

EXPORTS = ["kai_core_create", "kai_core_destroy", "kai_session_open", "kai_queue_shares", "kai_action_execute", "kai_best_node", "kai_best_nodes", "kai_ordered_nodes", "kai_ops_apply", "kai_stmt_begin", "kai_stmt_apply", "kai_stmt_checkpoint", "kai_stmt_rollback", "kai_stmt_discard", "kai_stmt_commit", "kai_stmt_place", "kai_stale_gang_eviction", "kai_job_order", "kai_subset_nodes", "kai_subset_nodes_scored", "kai_ordered_nodes_scored",
           "kai_pod_states", "kai_node_states", "kai_pod_gpu_groups", "kai_shard_attach", "kai_shard_attach_host", "kai_shard_rccl_id", "kai_shard_attach_rccl", "kai_shard_allgather_probe", "kai_action_stats_get", "kai_session_reset", "kai_session_update", "kai_session_update_rows", "kai_core_set_now", "kai_session_close", "kai_last_error", "kai_version"]


_SCORE_ROW_DTYPE = np.dtype([("level_row", "<i4"), ("n_scored", "<i4")])  # kai_topo_score_row
_OP_DTYPE = np.dtype([("seq", "<i8"), ("kind", "<i4"), ("pod", "<i4"), ("node", "<i4"), ("job", "<i4"), ("stmt", "<i4"), ("pad", "<i4")])  # kai_op (include/kai_core.h)


def delta_struct(pods, status, node, gpu_group=None, nodes=None, node_flags=None, node_allocatable=None, version=abi.DELTA_VERSION):
    """A kai_session_delta and the numpy arrays it points into (keep them alive while the struct is in use); None = a NULL array."""
    def arr(x, dt):
        return None if x is None else np.ascontiguousarray(x, dtype=dt)
    keep = [arr(pods, np.int32), arr(status, np.int32), arr(node, np.int32), arr(gpu_group, np.int32), arr(nodes, np.int32), arr(node_flags, np.uint32),
            arr(node_allocatable, np.float64)]
    def ptr(x, ct):
        return None if x is None else x.ctypes.data_as(C.POINTER(ct))
    d = abi.KaiSessionDelta()
    d.version = version
    d.n_pods = 0 if keep[0] is None else len(keep[0])
    d.pod, d.pod_status, d.pod_node, d.pod_gpu_group = ptr(keep[0], C.c_int32), ptr(keep[1], C.c_int32), ptr(keep[2], C.c_int32), ptr(keep[3], C.c_int32)
    d.n_nodes = 0 if keep[4] is None else len(keep[4])
    d.node, d.node_flags, d.node_allocatable = ptr(keep[4], C.c_int32), ptr(keep[5], C.c_uint32), ptr(keep[6], C.c_double)
    return d, keep


def rows_struct(now_ns=None, queues=None, queue_deserved=None, queue_limit=None, queue_oqw=None, queue_usage=None, queue_priority=None,
                queue_preempt_min_runtime_ns=None, queue_reclaim_min_runtime_ns=None, jobs=None, job_last_start_ns=None, version=abi.ROWS_VERSION, fields=None):
    """A kai_session_rows and the numpy arrays it points into (keep them alive while the struct is in use); None = a NULL array.
    The four queue quantities are [3][len(queues)]."""
    def arr(x, dt):
        return None if x is None else np.ascontiguousarray(x, dtype=dt)
    def ptr(x, ct):
        return None if x is None else x.ctypes.data_as(C.POINTER(ct))
    q, j = arr(queues, np.int32), arr(jobs, np.int32)
    f64 = [arr(x, np.float64) for x in (queue_deserved, queue_limit, queue_oqw, queue_usage)]
    for x in f64:
        assert x is None or x.size == 3 * (0 if q is None else len(q)), "a queue quantity is [3][len(queues)]"
    prio, pmr, rmr, jls = arr(queue_priority, np.int32), arr(queue_preempt_min_runtime_ns, np.int64), arr(queue_reclaim_min_runtime_ns, np.int64), arr(job_last_start_ns, np.int64)
    r = abi.KaiSessionRows()
    r.version = version
    r.fields = (abi.ROWS_HAS_NOW if now_ns is not None else 0) if fields is None else fields
    r.now_ns = 0 if now_ns is None else int(now_ns)
    r.n_queues = 0 if q is None else len(q)
    r.queue = ptr(q, C.c_int32)
    r.queue_deserved, r.queue_limit, r.queue_oqw, r.queue_usage = (ptr(x, C.c_double) for x in f64)
    r.queue_priority, r.queue_preempt_min_runtime_ns, r.queue_reclaim_min_runtime_ns = ptr(prio, C.c_int32), ptr(pmr, C.c_int64), ptr(rmr, C.c_int64)
    r.n_jobs = 0 if j is None else len(j)
    r.job, r.job_last_start_ns = ptr(j, C.c_int32), ptr(jls, C.c_int64)
    return r, [q, j, prio, pmr, rmr, jls] + f64


class KaiError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__(f"kai_core status {code} ({abi.STATUS_TEXT.get(code, '?')}): {detail}")


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)  # kai_allgather_fn (include/kai_core.h)
_lib = None
_hip = None


def _hip_runtime():
    """libamdhip64 through ctypes: device-to-device copies between the library's exchange buffers and torch's tensors."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipDeviceSynchronize.argtypes = []
        _hip.hipDeviceSynchronize.restype = C.c_int
    return _hip


def load_library(path: str = LIB_PATH):
    """dlopen libkai_core.so and declare prototypes.  Raises if the HIP extension was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing — build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                                "the scheduling-cycle core has no non-HIP implementation")
    lib = C.CDLL(path)
    lib.kai_version.restype = C.c_char_p
    lib.kai_last_error.restype = C.c_char_p
    lib.kai_last_error.argtypes = [C.c_void_p]
    lib.kai_core_create.argtypes = [C.POINTER(abi.KaiConfig), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    lib.kai_core_destroy.argtypes = [C.c_void_p]
    lib.kai_session_open.argtypes = [C.c_void_p, C.POINTER(abi.KaiSnapshotSoA)]
    lib.kai_session_close.argtypes = [C.c_void_p]
    lib.kai_shard_attach.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]
    lib.kai_shard_attach_host.argtypes = [C.c_void_p, ALLGATHER_FN, C.c_void_p]
    lib.kai_shard_rccl_id.argtypes = [C.c_void_p, C.c_void_p]
    lib.kai_shard_attach_rccl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.kai_shard_allgather_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.kai_pod_gpu_groups.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    lib.kai_session_reset.argtypes = [C.c_void_p]
    lib.kai_session_update.argtypes = [C.c_void_p, C.POINTER(abi.KaiSessionDelta)]
    lib.kai_session_update_rows.argtypes = [C.c_void_p, C.POINTER(abi.KaiSessionDelta), C.POINTER(abi.KaiSessionRows)]
    lib.kai_core_set_now.argtypes = [C.c_void_p, C.c_int64]
    lib.kai_queue_shares.argtypes = [C.c_void_p, C.POINTER(abi.KaiQueueShare), C.c_int]
    lib.kai_action_execute.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.KaiOp), C.c_int64, C.POINTER(C.c_int64)]
    lib.kai_best_node.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int)]
    lib.kai_best_nodes.argtypes = [C.c_void_p, C.POINTER(abi.KaiNodeQuery), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(abi.KaiNodeAnswer)]
    lib.kai_ordered_nodes.argtypes = [C.c_void_p, C.POINTER(abi.KaiNodeQuery), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.POINTER(abi.KaiNodeAnswer), C.POINTER(C.c_int32)]
    lib.kai_ops_apply.argtypes = [C.c_void_p, C.POINTER(abi.KaiOp), C.c_int64, C.c_uint32, C.POINTER(abi.KaiApplyResult)]
    lib.kai_stmt_begin.argtypes = [C.c_void_p, C.c_uint32]
    lib.kai_stmt_apply.argtypes = [C.c_void_p, C.POINTER(abi.KaiOp), C.c_int64, C.c_uint32, C.POINTER(abi.KaiStmtResult)]
    lib.kai_stmt_checkpoint.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.kai_stmt_rollback.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(abi.KaiStmtResult)]
    lib.kai_stmt_discard.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(abi.KaiStmtResult)]
    lib.kai_stmt_commit.argtypes = [C.c_void_p, C.POINTER(abi.KaiOp), C.c_int64, C.POINTER(C.c_int64), C.POINTER(abi.KaiStmtResult)]
    lib.kai_stmt_place.argtypes = [C.c_void_p, C.POINTER(abi.KaiPlaceParams), C.POINTER(abi.KaiPlaceGang), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                   C.POINTER(C.c_uint32), C.c_int32, C.POINTER(abi.KaiTopoScoreRow), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(abi.KaiPlaceAnswer), C.POINTER(C.c_int32),
                                   C.POINTER(abi.KaiOp), C.c_int64, C.POINTER(C.c_int64), C.POINTER(abi.KaiStmtResult)]
    lib.kai_stale_gang_eviction.argtypes = [C.c_void_p, C.POINTER(abi.KaiStaleParams), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(abi.KaiOp), C.c_int64,
                                            C.POINTER(C.c_int64), C.POINTER(abi.KaiStaleResult)]
    lib.kai_job_order.argtypes = [C.c_void_p, C.POINTER(abi.KaiJobOrderParams), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(abi.KaiJobOrderResult)]
    lib.kai_subset_nodes.argtypes = [C.c_void_p, C.POINTER(abi.KaiSubsetParams), C.POINTER(abi.KaiSubsetQuery), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(abi.KaiSubsetAnswer),
                                     C.POINTER(abi.KaiNodeSet), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(abi.KaiSubsetResult)]
    lib.kai_subset_nodes_scored.argtypes = [C.c_void_p, C.POINTER(abi.KaiSubsetParams), C.POINTER(abi.KaiSubsetQuery), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(abi.KaiSubsetAnswer),
                                            C.POINTER(abi.KaiNodeSet), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(abi.KaiTopoScoreRow), C.POINTER(C.c_uint8),
                                            C.POINTER(abi.KaiSubsetResult)]
    lib.kai_ordered_nodes_scored.argtypes = [C.c_void_p, C.POINTER(abi.KaiScoredQuery), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(abi.KaiTopoScoreRow), C.POINTER(C.c_uint8), C.c_int32,
                                             C.c_int32, C.POINTER(abi.KaiNodeAnswer), C.POINTER(C.c_int32)]
    lib.kai_pod_states.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]
    lib.kai_node_states.argtypes = [C.c_void_p, C.POINTER(abi.KaiNodeState), C.c_int]
    lib.kai_action_stats_get.argtypes = [C.c_void_p, C.POINTER(abi.KaiActionStats)]
    for name in EXPORTS:
        if name not in ("kai_version", "kai_last_error"):
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


class KaiCore:
    """One handle = one GPU.  `world` > 1: this process is rank `rank` of a group that shards the NODE axis of one session over the GPUs of one
    node (one process per GPU, every rank opens the same snapshot and makes the same calls).  The group's exchange step is an
    all-gather of a few KB per rank: `allgather(send_ptr, recv_ptr, nbytes_per_rank)` on the library's device buffers, by default
    torch.distributed.all_gather_into_tensor on the default process group (backend "nccl" = RCCL over xGMI on the GPU box)."""

    def __init__(self, cfg: abi.KaiConfig | None = None, gpu_ids=(0,), world: int = 1, rank: int = 0, offers_per_class: int = 0, allgather=None, host_allgather=None):
        self.lib = load_library()
        self.cfg = cfg or abi.default_config()
        self.handle = C.c_void_p()
        self.world, self.rank = int(world), int(rank)
        ids = (C.c_int * 1)(gpu_ids[0])
        rc = self.lib.kai_core_create(C.byref(self.cfg), self.world, ids, C.byref(self.handle))
        if rc != 0:
            raise KaiError(rc, "kai_core_create")
        if isinstance(allgather, str) and allgather == "rccl":
            # the library's own communicator (kai_shard_attach_rccl): rank 0 draws the id, the default process group carries it to the others, the exchange itself
            # is an ncclAllGather the library issues on its stream between its kernels
            self._attach_rccl(int(offers_per_class))
        elif self.world > 1:
            self._user_allgather = allgather
            self._stage = None
            self._cb = ALLGATHER_FN(self._allgather)  # kept alive with the handle
            rc = self.lib.kai_shard_attach(self.handle, self.rank, self.world, int(offers_per_class), self._cb, None)
            if rc != 0:
                raise KaiError(rc, "kai_shard_attach")

        if self.world > 1 and host_allgather is not None:
            # the victim actions' waves over the ranks (kai_shard_attach_host): host_allgather(send_ptr, recv_ptr, nbytes_per_rank) on HOST memory, called while the
            # action's kernel runs (it must not synchronise the device); True = torch.distributed on CPU tensors of a gloo group `host_group` (default group if gloo)
            self._host_ag = host_allgather
            self._hcb = ALLGATHER_FN(self._host_allgather)
            rc = self.lib.kai_shard_attach_host(self.handle, self._hcb, None)
            if rc != 0:
                raise KaiError(rc, "kai_shard_attach_host")

    host_group = None  # the process group host_allgather=True uses (a gloo group beside an nccl default group)

    def _host_allgather(self, user, send, recv, nbytes):
        try:
            if callable(self._host_ag):
                return int(self._host_ag(send, recv, nbytes) or 0)
            import numpy as np
            import torch
            import torch.distributed as dist
            s = torch.from_numpy(np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,)))
            r = torch.from_numpy(np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(nbytes * self.world,)))
            dist.all_gather_into_tensor(r, s, group=self.host_group)
            return 0
        except Exception:  # a ctypes callback must not raise
            import traceback
            traceback.print_exc()
            return 1

    def _attach_rccl(self, offers_per_class):
        idbuf = (C.c_ubyte * 128)()
        if self.rank == 0:
            rc = self.lib.kai_shard_rccl_id(self.handle, idbuf)
            if rc != 0:
                raise KaiError(rc, self.lib.kai_last_error(self.handle).decode())
        if self.world > 1:
            import torch
            import torch.distributed as dist
            t = torch.tensor(list(bytes(idbuf)), dtype=torch.uint8, device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.broadcast(t, 0)
            idbuf = (C.c_ubyte * 128)(*t.cpu().tolist())
        rc = self.lib.kai_shard_attach_rccl(self.handle, self.rank, self.world, offers_per_class, idbuf)
        if rc != 0:
            raise KaiError(rc, self.lib.kai_last_error(self.handle).decode())

    def _allgather(self, user, send, recv, nbytes):
        try:
            if self._user_allgather is not None:
                return int(self._user_allgather(send, recv, nbytes) or 0)
            import torch
            import torch.distributed as dist
            hip = _hip_runtime()
            on_host = dist.get_backend() != "nccl"  # a gloo group (rehearsal of the multi-process path without RCCL): staged through host memory
            if self._stage is None or self._stage[0].numel() != nbytes:  # torch-owned staging tensors: the collective runs on memory torch knows
                dev = "cpu" if on_host else "cuda"
                self._stage = (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes * self.world, dtype=torch.uint8, device=dev))
            s, r = self._stage
            if hip.hipMemcpy(C.c_void_p(s.data_ptr()), C.c_void_p(send), C.c_size_t(nbytes), 2 if on_host else 3) != 0:  # hipMemcpyDeviceToHost / DeviceToDevice
                return 1
            dist.all_gather_into_tensor(r, s)
            if not on_host: torch.cuda.synchronize()
            if hip.hipMemcpy(C.c_void_p(recv), C.c_void_p(r.data_ptr()), C.c_size_t(nbytes * self.world), 1 if on_host else 3) != 0:
                return 1
            # the library goes on with kernels on its own non-blocking stream, which has no implicit order with the null stream this copy ran on
            return 0 if hip.hipDeviceSynchronize() == 0 else 1
        except Exception:  # a ctypes callback must not raise
            import traceback
            traceback.print_exc()
            return 1

    def _check(self, rc):
        if rc != 0:
            raise KaiError(rc, self.lib.kai_last_error(self.handle).decode())

    def set_now(self, now_ns: int):
        """kai_core_set_now: the cycle's clock, at once on an open session and for every later open / reset / update of this handle."""
        self._check(self.lib.kai_core_set_now(self.handle, int(now_ns)))
        self.cfg = abi.copy_config(self.cfg)  # (the caller's structure stays as it was handed in)
        self.cfg.now_ns = int(now_ns)

    def open_session(self, snap: abi.Snapshot) -> "Session":
        s = snap.as_struct()
        self._check(self.lib.kai_session_open(self.handle, C.byref(s)))
        return Session(self, snap)

    def destroy(self):
        if self.handle:
            self.lib.kai_core_destroy(self.handle)
            self.handle = C.c_void_p()

    def _ops_buffer(self, cap: int):
        """The caller-owned `ops_out` array of kai_action_execute: one per handle, kept across sessions (untouched pages cost nothing; a fresh 68 MB array per session of config 5 would)."""
        buf = getattr(self, "_ops_buf", None)
        if buf is None or len(buf) < cap:
            buf = self._ops_buf = np.empty(cap, _OP_DTYPE)
        return buf

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.destroy()


class Session:
    """An open scheduling session resident in HBM."""

    def __init__(self, core: KaiCore, snap: abi.Snapshot):
        self.core, self.snap = core, snap

    def execute(self, action: str | int, copy: bool = True):
        """Run one Action; returns the committed operations [(kind, pod, node, job)] in commit order.

        `copy=False` returns a view of the handle's output buffer (the caller-owned `ops_out` of the C ABI): valid until the next `execute` on this handle."""
        lib, h = self.core.lib, self.core.handle
        act = abi.ACTIONS[action] if isinstance(action, str) else int(action)
        cap = 2 * self.snap.n_pods + 64
        ops = self.core._ops_buffer(cap)
        n = C.c_int64(0)
        self.core._check(lib.kai_action_execute(h, act, ops.ctypes.data_as(C.POINTER(abi.KaiOp)), cap, C.byref(n)))
        out = ops[:n.value]
        if not copy:
            return out
        # (a flat byte copy: numpy copies a structured array record by record, 3.5 ms for config 5's 150 k operations)
        return out.view(np.uint8).copy().view(_OP_DTYPE)

    def best_node(self, pod: int, pipeline_only: bool = False, nodeset=None):
        """Session.OrderedNodesByTask + FittingNode for one task; `nodeset` = iterable of node indices (None = all nodes)."""
        node, pipe = C.c_int32(-1), C.c_int(0)
        bits = None
        if nodeset is not None:
            words = np.zeros(max((self.snap.n_nodes + 31) // 32, 1), np.uint32)
            for n in nodeset:
                words[n >> 5] |= np.uint32(1 << (n & 31))
            bits = words.ctypes.data_as(C.POINTER(C.c_uint32))
        self.core._check(self.core.lib.kai_best_node(self.core.handle, pod, bits, int(pipeline_only), C.byref(node), C.byref(pipe)))
        return node.value, bool(pipe.value)

    def _node_queries(self, pods, nodesets, nodeset_of, pipeline_only):
        """The arguments best_nodes and ordered_nodes share, as kai_node_query records and node-set rows: (q, words, n_sets)."""
        pods = np.ascontiguousarray(pods, dtype=np.int32).ravel()
        M, N = len(pods), self.snap.n_nodes
        W = (N + 31) // 32
        sets = [] if nodesets is None else list(nodesets)
        words = np.zeros((max(len(sets), 1), max(W, 1)), np.uint32)
        for s, ns in enumerate(sets):
            ns = np.asarray(ns)
            idx = np.nonzero(ns)[0] if ns.dtype == np.bool_ else ns.astype(np.int64).ravel()
            if ns.dtype == np.bool_ and len(ns) != N:
                raise ValueError("a boolean node-set mask has one entry per node")
            if len(idx) and (idx.min() < 0 or idx.max() >= N):
                raise ValueError("node index out of range in a node set")
            np.bitwise_or.at(words[s], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
        q = np.zeros(M, dtype=np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("pad", "<i4")]))  # kai_node_query
        q["pod"] = pods
        q["nodeset"] = -1 if nodeset_of is None else np.array([-1 if s is None else int(s) for s in np.asarray(nodeset_of, dtype=object).ravel()], dtype=np.int32)
        if pipeline_only is not None:
            q["flags"] = np.where(np.broadcast_to(np.asarray(pipeline_only, dtype=bool), (M,)), abi.QUERY_PIPELINE_ONLY, 0)
        return q, words, len(sets)

    def best_nodes(self, pods, nodesets=None, nodeset_of=None, pipeline_only=None):
        """kai_best_nodes: best_node for many tasks in one chip-wide pass.  pods: pod indices; nodesets: node sets as index lists or boolean masks over the
        nodes; nodeset_of: per pod its set in `nodesets` (-1 / None = all nodes); pipeline_only: one bool for all or one per pod.
        Returns (node, is_pipeline): an int32 array (-1 = nothing fits) and a bool array."""
        q, words, n_sets = self._node_queries(pods, nodesets, nodeset_of, pipeline_only)
        M = len(q)
        out = np.zeros(M, dtype=np.dtype([("node", "<i4"), ("is_pipeline", "<i4")]))  # kai_node_answer
        self.core._check(self.core.lib.kai_best_nodes(self.core.handle, q.ctypes.data_as(C.POINTER(abi.KaiNodeQuery)), M,
                                                      words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_sets else None, n_sets,
                                                      out.ctypes.data_as(C.POINTER(abi.KaiNodeAnswer))))
        return out["node"].copy(), out["is_pipeline"].astype(bool)

    def ordered_nodes(self, pods, k, nodesets=None, nodeset_of=None, pipeline_only=None):
        """kai_ordered_nodes: per task the first k (1 .. abi.ORDERED_MAX_K) nodes of Session.OrderedNodesByTask that pass FittingNode, best first — the list the
        reference's allocation walks, of which best_nodes answers the head.  The arguments are best_nodes'.
        Returns (node [M, k] int32, is_pipeline [M, k] bool, count [M] int32): row i holds count[i] nodes, then -1 / False."""
        q, words, n_sets = self._node_queries(pods, nodesets, nodeset_of, pipeline_only)
        M, k = len(q), int(k)
        out = np.zeros((M, max(k, 1)), dtype=np.dtype([("node", "<i4"), ("is_pipeline", "<i4")]))  # kai_node_answer
        count = np.zeros(max(M, 1), np.int32)
        self.core._check(self.core.lib.kai_ordered_nodes(self.core.handle, q.ctypes.data_as(C.POINTER(abi.KaiNodeQuery)), M,
                                                         words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_sets else None, n_sets, k,
                                                         out.ctypes.data_as(C.POINTER(abi.KaiNodeAnswer)), count.ctypes.data_as(C.POINTER(C.c_int32))))
        return out["node"].copy(), out["is_pipeline"].astype(bool), count[:M]

    def ordered_nodes_scored(self, pods, k, nodesets=None, nodeset_of=None, score_rows=None, deciles=None, scores_of=None, pipeline_only=None):
        """kai_ordered_nodes_scored: ordered_nodes with the topology plugin's node scores.  score_rows, deciles: what subset_nodes_scored returned (any rows of it, in
        any order); scores_of: per pod its row in them (-1 / None = none: the pod is answered as ordered_nodes answers it).  A node whose domain at the row's level has
        no score is dropped; the others get decile x abi.TOPO_SCORE_UNIT on top of their score.  Returns what ordered_nodes returns."""
        q, words, n_sets = self._node_queries(pods, nodesets, nodeset_of, pipeline_only)
        M, k = len(q), int(k)
        D = int(self.snap.arrays["domain_level"].shape[0]) if "domain_level" in self.snap.arrays else 0  # n_domains
        rows = np.zeros(0, _SCORE_ROW_DTYPE) if score_rows is None else np.ascontiguousarray(score_rows, dtype=_SCORE_ROW_DTYPE).ravel()
        dec = np.ascontiguousarray(np.zeros((len(rows), D), np.uint8) if deciles is None else deciles, dtype=np.uint8).reshape(len(rows), D)
        q["pad"] = -1 if scores_of is None else np.array([-1 if s is None else int(s) for s in np.asarray(scores_of, dtype=object).ravel()], dtype=np.int32)  # kai_scored_query.scores
        out = np.zeros((M, max(k, 1)), dtype=np.dtype([("node", "<i4"), ("is_pipeline", "<i4")]))  # kai_node_answer
        count = np.zeros(max(M, 1), np.int32)
        pad = np.zeros(1, np.uint8)  # (an array without elements has no address to pass)
        self.core._check(self.core.lib.kai_ordered_nodes_scored(self.core.handle, q.ctypes.data_as(C.POINTER(abi.KaiScoredQuery)), M,
                                                                words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_sets else None, n_sets,
                                                                rows.ctypes.data_as(C.POINTER(abi.KaiTopoScoreRow)) if len(rows) else None,
                                                                (dec if dec.size else pad).ctypes.data_as(C.POINTER(C.c_uint8)) if len(rows) else None, len(rows), k,
                                                                out.ctypes.data_as(C.POINTER(abi.KaiNodeAnswer)), count.ctypes.data_as(C.POINTER(C.c_int32))))
        return out["node"].copy(), out["is_pipeline"].astype(bool), count[:M]

    def apply_ops(self, ops, check_only: bool = False, engine_path: bool = False):
        """kai_ops_apply: committed operations taken back into the session, as framework.Statement applies and commits them — `ops` is the array `execute` returns
        (of this or another handle), or any array of kai_op records (seq and job are not read).  check_only: validate, write nothing; engine_path: take the engine
        walk even where the chip-wide path qualifies.  Returns the kai_apply_result; a refusal raises KaiError with the result as its `.result`."""
        arr = np.ascontiguousarray(ops, dtype=_OP_DTYPE)
        res = abi.KaiApplyResult()
        flags = (abi.APPLY_CHECK_ONLY if check_only else 0) | (abi.APPLY_ENGINE_PATH if engine_path else 0)
        rc = self.core.lib.kai_ops_apply(self.core.handle, arr.ctypes.data_as(C.POINTER(abi.KaiOp)) if len(arr) else None, len(arr), flags, C.byref(res))
        if rc != 0:
            err = KaiError(rc, self.core.lib.kai_last_error(self.core.handle).decode())
            err.result = res
            raise err
        return res

    def statement(self) -> "Statement":
        """kai_stmt_begin: the session's one open (uncommitted) Statement — apply / checkpoint / rollback / discard / commit.  As a context manager it discards on an
        exception and on leaving the block uncommitted."""
        return Statement(self)

    def stale_gang_eviction(self, stale_since, grace_ns: int, dry_run: bool = False):
        """kai_stale_gang_eviction: the stalegangeviction action against the session's current state, at the handle's clock (KaiCore.set_now).  stale_since: per job
        StalenessInfo.TimeStamp in ns, 0 = nil (not modified); grace_ns < 0: never evict; dry_run: decide and report, the session is not written.
        Returns (ops, stale_since, stale, result): the evictions as kai_op records in ascending pod index, the new timestamps, StalenessInfo.Stale per job as a bool
        array, and the kai_stale_result."""
        J, P = self.snap.n_jobs, self.snap.n_pods
        since = np.zeros(max(J, 1), np.int64)
        since[:J] = np.asarray(stale_since, dtype=np.int64).ravel()
        stale = np.zeros(max(J, 1), np.uint8)
        ops = np.zeros(max(P, 1), _OP_DTYPE)
        n, res = C.c_int64(0), abi.KaiStaleResult()
        params = abi.KaiStaleParams(abi.STALE_VERSION, abi.STALE_DRY_RUN if dry_run else 0, int(grace_ns))
        self.core._check(self.core.lib.kai_stale_gang_eviction(self.core.handle, C.byref(params), since.ctypes.data_as(C.POINTER(C.c_int64)), stale.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                               ops.ctypes.data_as(C.POINTER(abi.KaiOp)), P, C.byref(n), C.byref(res)))
        return ops[:n.value].copy(), since[:J], stale[:J].astype(bool), res

    def job_order(self, depth: int = 0, engine_path: bool = False):
        """kai_job_order: the pop order of the queued jobs at the session's current state (what the reflectjoborder plugin serves), nothing allocated between pops.
        depth: 0 = the config's allocate queue depth, -1 = infinite, > 0 = that many jobs per leaf queue; engine_path: the heap walk even where the chip-wide path
        qualifies.  Returns (order, job_pos, job_queue_pos, result): the job indices in pop order, every job's position in it and among the jobs of its own leaf queue
        (-1: not in the order), and the kai_job_order_result."""
        J = self.snap.n_jobs
        order, pos, qpos = np.zeros(max(J, 1), np.int32), np.full(max(J, 1), -1, np.int32), np.full(max(J, 1), -1, np.int32)
        n, res = C.c_int32(0), abi.KaiJobOrderResult()
        params = abi.KaiJobOrderParams(abi.JOB_ORDER_VERSION, abi.JOB_ORDER_ENGINE_PATH if engine_path else 0, int(depth), 0)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self.core._check(self.core.lib.kai_job_order(self.core.handle, C.byref(params), ip(order), J, C.byref(n), ip(pos), ip(qpos), C.byref(res)))
        return order[:n.value].copy(), pos[:J], qpos[:J], res

    def subset_nodes(self, jobs, groups=None, podsets=None, nodesets=None, nodeset_of=None, engine_path: bool = False, bitmaps: bool = True):
        """kai_subset_nodes: the topology plugin's subSetNodesFn for many jobs, sub-groups or pod-sets at the session's current state.  jobs: job indices; groups /
        podsets: per query a SubGroupSet or a pod-set of the job (-1 / None: the job's root sub-group set; at most one of the two per query); nodesets, nodeset_of:
        the parent node sets, as for best_nodes; engine_path: the engine walk even where the chip-wide path qualifies; bitmaps: also return the sets' nodes.
        Returns (answers, sets, masks, result): the kai_subset_answer and kai_node_set records as structured arrays (the sets of query i are
        sets[answers["first"][i] : answers["first"][i] + answers["n_sets"][i]], in the order the action tries them), the sets' nodes as a bool array [n_sets, N]
        (None without bitmaps; a row can be passed as a node set of best_nodes / ordered_nodes), and the kai_subset_result."""
        return self._subset_nodes(False, jobs, groups, podsets, nodesets, nodeset_of, engine_path, bitmaps)

    def subset_nodes_scored(self, jobs, groups=None, podsets=None, nodesets=None, nodeset_of=None, engine_path: bool = False, bitmaps: bool = True):
        """kai_subset_nodes_scored: subset_nodes with the topology plugin's node scores.  Returns (answers, sets, masks, score_rows, deciles, result): the first three and the
        last as subset_nodes returns them; score_rows: a structured array (level_row, n_scored) per query — level_row the node_domain row a node's domain is read from,
        abi.TOPO_SCORES_NONE where the reference records nothing for the sub-group (a task then uses the nearest ancestor group's row that is not NONE: the caller's
        choice), abi.TOPO_SCORES_EMPTY for a preferred level the topology does not have; deciles: uint8 [M, n_domains], floor((idx + 1) / n_scored * 10) for the scored
        domains, abi.TOPO_NO_SCORE elsewhere.  Both go into ordered_nodes_scored as they are."""
        return self._subset_nodes(True, jobs, groups, podsets, nodesets, nodeset_of, engine_path, bitmaps)

    def _subset_nodes(self, scored, jobs, groups, podsets, nodesets, nodeset_of, engine_path, bitmaps):
        """The call subset_nodes and subset_nodes_scored share (scored: with the score rows and deciles)."""
        jobs = np.ascontiguousarray(jobs, dtype=np.int32).ravel()
        M, N = len(jobs), self.snap.n_nodes
        W = max((N + 31) // 32, 1)
        _q, words, n_rows = self._node_queries(np.zeros(M, np.int32), nodesets, nodeset_of, None)
        per = lambda v: np.full(M, -1, np.int32) if v is None else np.array([-1 if x is None else int(x) for x in np.asarray(v, dtype=object).ravel()], dtype=np.int32)
        q = np.zeros(M, dtype=np.dtype([("job", "<i4"), ("group", "<i4"), ("podset", "<i4"), ("nodeset", "<i4")]))  # kai_subset_query
        q["job"], q["group"], q["podset"], q["nodeset"] = jobs, per(groups), per(podsets), _q["nodeset"]
        ans = np.zeros(max(M, 1), dtype=np.dtype([("status", "<i4"), ("n_sets", "<i4"), ("first", "<i4"), ("tasks", "<i4"), ("common_domain", "<i4"), ("pad", "<i4")]))  # kai_subset_answer
        set_dt = np.dtype([("domain", "<i4"), ("level", "<i4"), ("allocatable_pods", "<i4"), ("n_nodes", "<i4")])  # kai_node_set
        params = abi.KaiSubsetParams(abi.SUBSET_VERSION, abi.SUBSET_ENGINE_PATH if engine_path else 0)
        n, res = C.c_int64(0), abi.KaiSubsetResult()
        cap = max(64, 8 * M)
        D = int(self.snap.arrays["domain_level"].shape[0]) if "domain_level" in self.snap.arrays else 0  # n_domains
        score_rows, deciles = np.zeros(max(M, 1), _SCORE_ROW_DTYPE), np.zeros((max(M, 1), max(D, 1)), np.uint8)
        tail = (score_rows.ctypes.data_as(C.POINTER(abi.KaiTopoScoreRow)), deciles.ctypes.data_as(C.POINTER(C.c_uint8))) if scored else ()
        fn = self.core.lib.kai_subset_nodes_scored if scored else self.core.lib.kai_subset_nodes
        for _ in range(2):  # the capacity protocol: where the first guess is too small the call says how many there are, and the second call has room
            sets = np.zeros(max(cap, 1), set_dt)
            maps = np.zeros((max(cap, 1), W), np.uint32) if bitmaps else None
            rc = fn(self.core.handle, C.byref(params), q.ctypes.data_as(C.POINTER(abi.KaiSubsetQuery)), M,
                    words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_rows else None, n_rows, ans.ctypes.data_as(C.POINTER(abi.KaiSubsetAnswer)),
                    sets.ctypes.data_as(C.POINTER(abi.KaiNodeSet)), cap, C.byref(n), maps.ctypes.data_as(C.POINTER(C.c_uint32)) if bitmaps else None, *tail, C.byref(res))
            if rc != -4 or n.value <= cap:  # KAI_ERR_CAPACITY
                break
            cap = int(n.value)
        self.core._check(rc)
        total = int(n.value)
        masks = None
        if bitmaps:
            bits = (maps[:total, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
            masks = bits.reshape(total, W * 32)[:, :N].astype(bool)
        if scored:
            return ans[:M], sets[:total].copy(), masks, score_rows[:M], np.ascontiguousarray(deciles[:M, :D]), res
        return ans[:M], sets[:total].copy(), masks, res

    def gpu_groups(self):
        """PodInfo.GPUGroups[0] of the active fraction pods (-1 elsewhere): kai_pod_gpu_groups."""
        P = self.snap.n_pods
        out = np.full(max(P, 1), -1, np.int32)
        self.core._check(self.core.lib.kai_pod_gpu_groups(self.core.handle, out.ctypes.data_as(C.POINTER(C.c_int32)), max(P, 1)))
        return out[:P]

    def queue_shares(self):
        Q = self.snap.n_queues
        out = (abi.KaiQueueShare * max(Q, 1))()
        self.core._check(self.core.lib.kai_queue_shares(self.core.handle, out, max(Q, 1)))
        res = {}
        for f in ("fair_share", "allocated", "allocated_non_preemptible", "request", "deserved", "max_allowed"):
            res[f] = np.array([[getattr(out[q], f)[r] for r in range(3)] for q in range(Q)], dtype=np.float64).reshape(Q, 3)
        return res

    def pod_states(self):
        P = self.snap.n_pods
        st, nd = np.zeros(max(P, 1), np.int32), np.zeros(max(P, 1), np.int32)
        self.core._check(self.core.lib.kai_pod_states(self.core.handle, st.ctypes.data_as(C.POINTER(C.c_int32)), nd.ctypes.data_as(C.POINTER(C.c_int32)), max(P, 1)))
        return st[:P], nd[:P]

    def node_states(self):
        N, R = self.snap.n_nodes, self.snap.n_res
        out = (abi.KaiNodeState * max(N, 1))()
        self.core._check(self.core.lib.kai_node_states(self.core.handle, out, max(N, 1)))
        raw = np.frombuffer(out, dtype=np.float64).reshape(max(N, 1), 3, abi.MAX_RES)
        return {"idle": raw[:N, 0, :R].copy(), "releasing": raw[:N, 1, :R].copy(), "used": raw[:N, 2, :R].copy()}

    def stats(self) -> abi.KaiActionStats:
        st = abi.KaiActionStats()
        self.core._check(self.core.lib.kai_action_stats_get(self.core.handle, C.byref(st)))
        return st

    def reset(self):
        """Re-open the session from the HBM-resident snapshot (no host traffic)."""
        self.core._check(self.core.lib.kai_session_reset(self.core.handle))

    def update(self, pods, status, node, gpu_group=None, nodes=None, node_flags=None, node_allocatable=None):
        """kai_session_update: apply a pod / node delta to the session's snapshot (the handle then equals one that opened S'; include/kai_core.h).
        pods / status / node: the changed pods, their new status and node (caller's index or -1); gpu_group: their new shared-GPU groups (None = unchanged);
        nodes: the changed nodes, with node_flags ([n]) and / or node_allocatable ([R][n]), None = unchanged.  On success self.snap becomes S'."""
        d, _keep = delta_struct(pods, status, node, gpu_group, nodes, node_flags, node_allocatable)
        self.core._check(self.core.lib.kai_session_update(self.core.handle, C.byref(d)))
        self.snap = abi.apply_delta(self.snap, pods, status, node, gpu_group, nodes, node_flags, node_allocatable)

    def update_rows(self, delta_args=None, rows_args=None):
        """kai_session_update_rows: a pod / node delta (keyword arguments of `update`, or None) and the rows (keyword arguments of rows_struct / abi.apply_rows, or
        None) applied in one pass.  On success self.snap becomes S' and the core's config cfg'."""
        d = keep = r = keep2 = None
        if delta_args is not None:
            d, keep = delta_struct(**delta_args)
        if rows_args is not None:
            r, keep2 = rows_struct(**rows_args)
        self.core._check(self.core.lib.kai_session_update_rows(self.core.handle, None if d is None else C.byref(d), None if r is None else C.byref(r)))
        if delta_args is not None:
            self.snap = abi.apply_delta(self.snap, **delta_args)
        if rows_args is not None:
            self.snap, self.core.cfg = abi.apply_rows(self.snap, self.core.cfg, **rows_args)

    def close(self):
        self.core.lib.kai_session_close(self.core.handle)


class Statement:
    """An open Statement on a session (kai_stmt_*, include/kai_core.h): operations applied without the commit, logged on the device, rolled back to a checkpoint,
    discarded or committed.  While it is open the session's queries and read-backs see the tentative state; actions, apply_ops and stale_gang_eviction are refused."""

    def __init__(self, ssn: Session):
        self.ssn, self.core, self.open = ssn, ssn.core, False
        self.core._check(self.core.lib.kai_stmt_begin(self.core.handle, abi.STMT_VERSION))
        self.open = True

    def _done(self, rc, res):
        if rc != 0:
            err = KaiError(rc, self.core.lib.kai_last_error(self.core.handle).decode())
            err.result = res
            raise err
        return res

    def apply(self, ops, check_only: bool = False, engine_path: bool = False):
        """kai_stmt_apply: `ops` as apply_ops takes them (stmt is not read); an allocated pod is left Allocated.  Returns the kai_stmt_result; a refusal raises KaiError
        with the result as its `.result` and leaves the Statement open as it was."""
        arr = np.ascontiguousarray(ops, dtype=_OP_DTYPE)
        res = abi.KaiStmtResult()
        flags = (abi.APPLY_CHECK_ONLY if check_only else 0) | (abi.APPLY_ENGINE_PATH if engine_path else 0)
        return self._done(self.core.lib.kai_stmt_apply(self.core.handle, arr.ctypes.data_as(C.POINTER(abi.KaiOp)) if len(arr) else None, len(arr), flags, C.byref(res)), res)

    def checkpoint(self) -> int:
        """kai_stmt_checkpoint: the log's length (no device call)."""
        cp = C.c_int64(0)
        self.core._check(self.core.lib.kai_stmt_checkpoint(self.core.handle, C.byref(cp)))
        return cp.value

    def rollback(self, cp: int, engine_path: bool = False):
        """kai_stmt_rollback: the operations behind checkpoint `cp` undone.  Returns the kai_stmt_result."""
        res = abi.KaiStmtResult()
        return self._done(self.core.lib.kai_stmt_rollback(self.core.handle, int(cp), abi.APPLY_ENGINE_PATH if engine_path else 0, C.byref(res)), res)

    def discard(self, engine_path: bool = False):
        """kai_stmt_discard: every operation undone, the Statement closed.  Returns the kai_stmt_result."""
        res = abi.KaiStmtResult()
        rc = self.core.lib.kai_stmt_discard(self.core.handle, abi.APPLY_ENGINE_PATH if engine_path else 0, C.byref(res))
        self.open = self.open and rc != 0
        return self._done(rc, res)

    def commit(self):
        """kai_stmt_commit: the surviving operations committed (allocated pods become Binding), the Statement closed.  Returns (ops, result): the operations as
        kai_op records — seq from 0, stmt 0, job filled, nodes in the caller's indices."""
        cap = self.checkpoint()
        ops = np.zeros(max(cap, 1), _OP_DTYPE)
        n, res = C.c_int64(0), abi.KaiStmtResult()
        rc = self.core.lib.kai_stmt_commit(self.core.handle, ops.ctypes.data_as(C.POINTER(abi.KaiOp)), cap, C.byref(n), C.byref(res))
        self.open = self.open and rc != 0
        self._done(rc, res)
        return ops[:n.value].copy(), res

    def place(self, gangs, nodesets=None, score_rows=None, deciles=None, pipeline_only: bool = False, engine_path: bool = False):
        """kai_stmt_place: whole gangs placed on their node sets in one call — per gang a checkpoint, its sets in order, per set its tasks in order, each on the best
        node of the set at the state its predecessors left; a set without a node for a task is rolled back and the next one is tried.
        gangs: (pods, sets) or (pods, sets, scores) per gang — pods in placement order, sets as indices into `nodesets` in the order they are tried (-1 / None = all
        nodes), scores a row of score_rows / deciles (subset_nodes_scored's outputs) or -1; nodesets: node sets as index lists or boolean masks (a row of subset_nodes'
        masks as it is).  Returns (answers, fail_at, ops, result): the kai_place_answer records; per gang an int32 array over its sets — the gang's index of the first
        task the set had no node for, len(pods) for the set that took it, -1 for a set that was not tried; the call's surviving operations as kai_op records (log order,
        seq = the position in the log); the kai_stmt_result.  A refusal raises KaiError with the result as its `.result` and leaves the Statement open as it was."""
        _q, words, n_rows = self.ssn._node_queries(np.zeros(0, np.int32), nodesets, None, None)
        G = len(gangs)
        gv = np.zeros(max(G, 1), dtype=np.dtype([("first_task", "<i4"), ("n_tasks", "<i4"), ("first_set", "<i4"), ("n_sets", "<i4"), ("scores", "<i4"), ("pad", "<i4")]))  # kai_place_gang
        tasks, sets = [], []
        for g, gang in enumerate(gangs):
            pods, ss = list(np.asarray(gang[0], dtype=np.int64).ravel()), [-1 if s is None else int(s) for s in np.asarray(gang[1], dtype=object).ravel()]
            gv[g] = (len(tasks), len(pods), len(sets), len(ss), int(gang[2]) if len(gang) > 2 and gang[2] is not None else -1, 0)
            tasks += pods; sets += ss
        tv, sv = np.array(tasks + [0], np.int32), np.array(sets + [0], np.int32)
        T, S = len(tasks), len(sets)
        n_sr = 0 if score_rows is None else len(score_rows)
        sr = np.ascontiguousarray(score_rows, dtype=_SCORE_ROW_DTYPE) if n_sr else None
        dc = np.ascontiguousarray(deciles, dtype=np.uint8) if n_sr else None
        ans = np.zeros(max(G, 1), dtype=np.dtype([("status", "<i4"), ("set", "<i4"), ("sets_tried", "<i4"), ("pad", "<i4"), ("first_op", "<i8"), ("n_ops", "<i8")]))  # kai_place_answer
        fail = np.full(max(S, 1), -1, np.int32)
        ops = np.zeros(max(T, 1), _OP_DTYPE)
        n, res = C.c_int64(0), abi.KaiStmtResult()
        params = abi.KaiPlaceParams(abi.PLACE_VERSION, (abi.PLACE_PIPELINE_ONLY if pipeline_only else 0) | (abi.APPLY_ENGINE_PATH if engine_path else 0))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = self.core.lib.kai_stmt_place(self.core.handle, C.byref(params), gv.ctypes.data_as(C.POINTER(abi.KaiPlaceGang)), G, ip(tv), T, ip(sv), S,
                                          words.ctypes.data_as(C.POINTER(C.c_uint32)) if n_rows else None, n_rows,
                                          sr.ctypes.data_as(C.POINTER(abi.KaiTopoScoreRow)) if n_sr else None, dc.ctypes.data_as(C.POINTER(C.c_uint8)) if n_sr else None, n_sr,
                                          ans.ctypes.data_as(C.POINTER(abi.KaiPlaceAnswer)), ip(fail), ops.ctypes.data_as(C.POINTER(abi.KaiOp)), T, C.byref(n), C.byref(res))
        self._done(rc, res)
        return ans[:G], [fail[gv["first_set"][g]: gv["first_set"][g] + gv["n_sets"][g]].copy() for g in range(G)], ops[:n.value].copy(), res

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.open:
            try:
                self.discard()
            except KaiError:
                if exc_type is None:
                    raise
                self.open = False  # (the session went with what raised: nothing is left to discard)
        return False
