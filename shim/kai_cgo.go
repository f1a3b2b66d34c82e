// Package gpucore routes the placement actions of the KAI scheduler (allocate, consolidation, reclaim, preempt) through
// libkai_core on an MI355X.  It is the reference-side binding of include/kai_core.h: a framework.Plugin that packs the
// session into the C ABI's structure-of-arrays at OnSessionOpen, and framework.Actions that run kai_action_execute and
// replay the committed operations through the real Statement, so that cache.Bind / Evict, fit errors, status updates
// and metrics stay on the Go side.
//
// Drop this file into pkg/scheduler/gpucore/ of NVIDIA/KAI-Scheduler (paths below are under pkg/scheduler/).  The build
// image of this repository has no Go toolchain, so the file is shipped as source, not compiled here; the host-side mirror
// that IS exercised is kai-scheduler_amd/core.py (same calls, same order) and the packing rules are pinned by
// tests/kai_testlib.py::case_to_snapshot and kai_ingest.cpp, which pack the same fields from the reference's fixtures
// and from snapshot.json.
package gpucore

/*
#cgo CFLAGS:  -I${SRCDIR}/../../../third_party/kai_core/include
#cgo LDFLAGS: -L${SRCDIR}/../../../third_party/kai_core/lib -lkai_core
#include <stdlib.h>
#include <string.h>
#include "kai_core.h"
*/
import "C"

import (
	"fmt"
	mathbits "math/bits"
	"sort"
	"time"
	"unsafe"

	v1 "k8s.io/api/core/v1"
	"k8s.io/apimachinery/pkg/types"

	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/actions/allocate"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/actions/consolidation"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/actions/preempt"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/actions/reclaim"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/actions/utils"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/common_info"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/eviction_info"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/node_info"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/pod_info"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/pod_status"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/podgroup_info"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/api/queue_info"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/framework"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/plugins/reflectjoborder"
	"github.com/NVIDIA/KAI-scheduler/pkg/scheduler/scheduler_util"
)

const nRes = 4 // cpu (milli), memory (bytes), gpu (devices), pods — api/resource_info/resource_vector.go:23-36.  Rows >= 4 (other scalar resources; MIG instance
// types with res_mig_gpus / res_mig_memory beside them, ABI v5) are laid out as kai_ingest.cpp does from the snapshot file; this shim packs the four base rows and leaves
// tasks with MIG instances to the fallback rule below.

var core *C.kai_core // one handle per scheduler process (= per scheduling shard)

// Init creates the device handle.  cfg mirrors conf.SchedulerParams and the plugin arguments the path reads.
func Init(cfg C.kai_config, gpu int) error {
	id := C.int(gpu)
	if rc := C.kai_core_create(&cfg, 1, &id, &core); rc != 0 {
		return fmt.Errorf("kai_core_create: status %d", int(rc))
	}
	return nil
}

// ------------------------------------------------------------------------------------------------ packed snapshot
// Everything the ABI takes lives in C memory (cgo forbids retaining Go pointers); freed at OnSessionClose.
type packedSnapshot struct {
	soa      C.kai_snapshot_soa
	allocs   []unsafe.Pointer
	pods     []*pod_info.PodInfo           // ABI pod index  -> task
	nodes    []*node_info.NodeInfo         // ABI node index -> node
	jobs     []*podgroup_info.PodGroupInfo // ABI job index  -> pod group
	classes  *staticClasses                // pod / node classes of the static Filters, shared-GPU group ids
	fallback bool                          // the rest of this cycle runs on the Go actions
}

func (p *packedSnapshot) free() {
	for _, a := range p.allocs {
		C.free(a)
	}
	p.allocs = nil
}

func carray[T any](p *packedSnapshot, n int) []T {
	var zero T
	sz := C.size_t(max(n, 1)) * C.size_t(unsafe.Sizeof(zero))
	mem := C.malloc(sz)
	C.memset(mem, 0, sz)
	p.allocs = append(p.allocs, mem)
	return unsafe.Slice((*T)(mem), max(n, 1))[:n:n]
}
func ptr[T any](s []T) *T {
	if len(s) == 0 {
		return nil
	}
	return &s[0]
}

// ranks of strings in byte-wise order: the reference's tie-breaks are Go string compares
// (framework/session.go:480-485 node names; framework/session_plugins.go:227-260 job / pod UIDs)
func rankStrings(keys []string) []C.uint32_t {
	idx := make([]int, len(keys))
	for i := range idx {
		idx[i] = i
	}
	sort.SliceStable(idx, func(a, b int) bool { return keys[idx[a]] < keys[idx[b]] })
	out := make([]C.uint32_t, len(keys))
	for r, i := range idx {
		out[i] = C.uint32_t(r)
	}
	return out
}

func statusBit(s pod_status.PodStatus) C.int32_t { // api/pod_status/pod_status.go:25-71 in declaration order
	switch s {
	case pod_status.Pending:
		return C.KAI_POD_PENDING
	case pod_status.Gated:
		return C.KAI_POD_GATED
	case pod_status.Allocated:
		return C.KAI_POD_ALLOCATED
	case pod_status.Pipelined:
		return C.KAI_POD_PIPELINED
	case pod_status.Binding:
		return C.KAI_POD_BINDING
	case pod_status.Bound:
		return C.KAI_POD_BOUND
	case pod_status.Running:
		return C.KAI_POD_RUNNING
	case pod_status.Releasing:
		return C.KAI_POD_RELEASING
	case pod_status.Succeeded:
		return C.KAI_POD_SUCCEEDED
	case pod_status.Failed:
		return C.KAI_POD_FAILED
	case pod_status.Deleted:
		return C.KAI_POD_DELETED
	}
	return C.KAI_POD_UNKNOWN
}

// podModelFlags: what the device path does not carry for this task (SURVEY §8b fallback rule; kai_ingest.cpp:592-611 sets the same bits from snapshot.json).
//   KAI_POD_CPU_FALLBACK   a state-dependent upstream predicate or a request kind without a device model: a PENDING pod with it makes kai_session_open decline
//   KAI_POD_GPU_UNMODELLED several fractional devices / DRA claims: an ACTIVE pod with it holds GPU state the node accounting would overstate, the session is declined
//   KAI_POD_LEGACY_MIG     a legacy MIG task (annotation-named instances): never scheduled, and its node takes no MIG request (node_info.go:315-359, 407-409)
// A fraction or MiB of ONE device (ABI v4 / v5) and MIG instance requests (resource rows >= 4) are described to the device and need no flag.
func podModelFlags(t *pod_info.PodInfo) C.uint32_t {
	var f C.uint32_t
	if t.IsLegacyMIGtask {
		f |= C.KAI_POD_LEGACY_MIG
	}
	multiFraction := t.ResReq.GetNumOfGpuDevices() > 1 && t.ResReq.IsFractionalRequest()
	dra := t.ResReq.GetDraGpusCount() > 0 || len(t.Pod.Spec.ResourceClaims) > 0
	if multiFraction || dra {
		f |= C.KAI_POD_CPU_FALLBACK | C.KAI_POD_GPU_UNMODELLED
	}
	if len(t.ResReq.MigResources()) > 0 {
		f |= C.KAI_POD_CPU_FALLBACK // this shim packs the four base resource rows only (nRes): MIG instance rows are laid out by the snapshot-file path
	}
	spec := t.Pod.Spec
	if spec.Affinity != nil && (spec.Affinity.PodAffinity != nil || spec.Affinity.PodAntiAffinity != nil) {
		f |= C.KAI_POD_CPU_FALLBACK
	}
	for _, cs := range [][]v1.Container{spec.Containers, spec.InitContainers} {
		for _, c := range cs {
			for _, port := range c.Ports {
				if port.HostPort != 0 {
					f |= C.KAI_POD_CPU_FALLBACK
				}
			}
		}
	}
	if len(t.GetAllStorageClaims()) > 0 {
		f |= C.KAI_POD_CPU_FALLBACK
	}
	return f
}

// packSnapshot: ssn.ClusterInfo (api/cluster_info.go:43-64, built by cache/cluster_info/cluster_info.go:118-228) ->
// kai_snapshot_soa, field by field as include/kai_core.h documents them.
func packSnapshot(ssn *framework.Session, params packParams) *packedSnapshot {
	p := &packedSnapshot{}
	ci := ssn.ClusterInfo
	s := &p.soa
	s.abi_version = C.KAI_ABI_VERSION
	s.n_res = nRes

	// ---- nodes, in map-iteration-independent (name) order; the library re-permutes by node_name_rank itself
	names := make([]string, 0, len(ci.Nodes))
	for name := range ci.Nodes {
		names = append(names, name)
	}
	sort.Strings(names)
	N := len(names)
	nodeIdx := make(map[string]int, N)
	alloc := carray[C.double](p, nRes*N)
	flags := carray[C.uint32_t](p, N)
	gpuCount := carray[C.int32_t](p, N)
	nodeClass := carray[C.int32_t](p, N)
	gpuMem := carray[C.int64_t](p, N)
	for i, name := range names {
		n := ci.Nodes[name]
		nodeIdx[name] = i
		p.nodes = append(p.nodes, n)
		alloc[0*N+i] = C.double(n.Allocatable.Cpu())
		alloc[1*N+i] = C.double(n.Allocatable.Memory())
		alloc[2*N+i] = C.double(n.Allocatable.GPUs())
		alloc[3*N+i] = C.double(n.Allocatable.Get(v1.ResourcePods))
		if err := scheduler_util.CheckNodeConditionPredicate(n.Node); err != nil { // scheduler_util/scheduler_utils.go:12-40
			flags[i] |= C.KAI_NODE_NOT_READY
		}
		if n.IsMIGEnabled() { // api/node_info/node_info.go:704-718
			flags[i] |= C.KAI_NODE_MIG_ENABLED
		}
		switch n.GetMigStrategy() { // :720-732
		case node_info.MigStrategyMixed:
			flags[i] |= C.KAI_NODE_MIG_MIXED
		case node_info.MigStrategySingle:
			flags[i] |= C.KAI_NODE_MIG_SINGLE
		}
		if n.HasDRAGPUs {
			flags[i] |= C.KAI_NODE_HAS_DRA_GPUS
		}
		if _, ok := n.Node.Labels[params.gpuWorkerLabel]; ok { // plugins/predicates/predicates.go:243-259
			flags[i] |= C.KAI_NODE_GPU_WORKER
		}
		if _, ok := n.Node.Labels[params.cpuWorkerLabel]; ok {
			flags[i] |= C.KAI_NODE_CPU_WORKER
		}
		gpuCount[i] = -1
		if c, ok := n.GetLabelGpuCount(); ok { // nvidia.com/gpu.count (node_info.go:619-640)
			gpuCount[i] = C.int32_t(c)
		}
		gpuMem[i] = C.int64_t(n.MemoryOfEveryGpuOnNode)
	}
	nodeRank := rankStrings(names)
	cNodeRank := carray[C.uint32_t](p, N)
	copy(cNodeRank, nodeRank)

	// ---- queues (leaf queues and departments share one index space); parents before use is not required
	qids := make([]string, 0, len(ci.Queues))
	for id := range ci.Queues {
		qids = append(qids, string(id))
	}
	sort.Strings(qids)
	Q := len(qids)
	queueIdx := make(map[string]int, Q)
	for i, id := range qids {
		queueIdx[id] = i
	}
	qParent := carray[C.int32_t](p, Q)
	qPrio := carray[C.int32_t](p, Q)
	qCreated := carray[C.int64_t](p, Q)
	qUID := carray[C.uint32_t](p, Q)
	qDeserved := carray[C.double](p, 3*Q)
	qLimit := carray[C.double](p, 3*Q)
	qOqw := carray[C.double](p, 3*Q)
	qUsage := carray[C.double](p, 3*Q)
	qPreMR := carray[C.int64_t](p, Q)
	qRecMR := carray[C.int64_t](p, Q)
	copy(qUID, rankStrings(qids))
	for i, id := range qids {
		q := ci.Queues[queue_info.QueueID(id)] // import alias of common_info.QueueID in the reference
		qParent[i] = -1
		if pi, ok := queueIdx[string(q.ParentQueue)]; ok && q.ParentQueue != "" {
			qParent[i] = C.int32_t(pi)
		}
		qPrio[i] = C.int32_t(q.Priority)
		qCreated[i] = C.int64_t(q.CreationTimestamp.UnixNano())
		for k, rq := range []queue_info.ResourceQuota{q.Resources.CPU, q.Resources.Memory, q.Resources.GPU} { // KAI_Q_CPU, _MEM, _GPU
			qDeserved[k*Q+i] = C.double(rq.Quota) // memory stays in the CRD's 10^6-byte units: the library applies proportion.go:327-328
			qLimit[k*Q+i] = C.double(rq.Limit)
			qOqw[k*Q+i] = C.double(rq.OverQuotaWeight)
		}
		if u, ok := ci.QueueResourceUsage.Queues[q.UID]; ok { // normalised historical usage (api/queue_info/quota_info.go)
			qUsage[0*Q+i], qUsage[1*Q+i], qUsage[2*Q+i] = C.double(u[v1.ResourceCPU]), C.double(u[v1.ResourceMemory]), C.double(u["nvidia.com/gpu"])
		}
		qPreMR[i], qRecMR[i] = -1, -1
		if q.PreemptMinRuntime != nil {
			qPreMR[i] = C.int64_t(q.PreemptMinRuntime.Duration.Nanoseconds())
		}
		if q.ReclaimMinRuntime != nil {
			qRecMR[i] = C.int64_t(q.ReclaimMinRuntime.Duration.Nanoseconds())
		}
	}

	// ---- jobs, pod-sets, pods: pods of one job contiguous, pod-sets of one job contiguous
	jids := make([]string, 0, len(ci.PodGroupInfos))
	for id := range ci.PodGroupInfos {
		jids = append(jids, string(id))
	}
	sort.Strings(jids)
	J := len(jids)
	P, S := 0, 0
	for _, id := range jids {
		job := ci.PodGroupInfos[podgroup_info.PodGroupID(id)]
		P += len(job.GetAllPodsMap())
		S += len(job.PodSets)
	}
	jQueue := carray[C.int32_t](p, J)
	jPrio := carray[C.int32_t](p, J)
	jPreempt := carray[C.int32_t](p, J)
	jCreated := carray[C.int64_t](p, J)
	jUID := carray[C.uint32_t](p, J)
	jFirstPod := carray[C.int32_t](p, J)
	jNPods := carray[C.int32_t](p, J)
	jFirstPS := carray[C.int32_t](p, J)
	jNPS := carray[C.int32_t](p, J)
	jSig := carray[C.int64_t](p, J)
	jLastStart := carray[C.int64_t](p, J)
	psJob := carray[C.int32_t](p, S)
	psMin := carray[C.int32_t](p, S)
	psRank := carray[C.uint32_t](p, S)
	req := carray[C.double](p, nRes*P)
	pJob := carray[C.int32_t](p, P)
	pPS := carray[C.int32_t](p, P)
	pStatus := carray[C.int32_t](p, P)
	pNode := carray[C.int32_t](p, P)
	pFlags := carray[C.uint32_t](p, P)
	pTaskPrio := carray[C.int32_t](p, P)
	pCreated := carray[C.int64_t](p, P)
	pUID := carray[C.uint32_t](p, P)
	pClass := carray[C.int32_t](p, P)
	pNominated := carray[C.int32_t](p, P)
	pPortion := carray[C.double](p, P)
	pGpuMem := carray[C.int64_t](p, P)
	pGroup := carray[C.int32_t](p, P)
	copy(jUID, rankStrings(jids))
	sigIDs := map[string]int64{}
	podUIDs := make([]string, 0, P)
	classes := newStaticClasses(p.nodes) // pod classes by constraint sub-tree, node classes by the labels / taints those constraints see
	p.classes = classes
	pi, si := 0, 0
	for j, id := range jids {
		job := ci.PodGroupInfos[podgroup_info.PodGroupID(id)]
		p.jobs = append(p.jobs, job)
		jQueue[j] = -1
		if qi, ok := queueIdx[string(job.Queue)]; ok {
			jQueue[j] = C.int32_t(qi)
		}
		jPrio[j] = C.int32_t(job.Priority)
		if job.IsPreemptibleJob() {
			jPreempt[j] = 1
		}
		jCreated[j] = C.int64_t(job.CreationTimestamp.UnixNano())
		sig := string(job.GetSchedulingConstraintsSignature()) // only equality is used (actions/common/minimal_job_comparison.go:15-44)
		if _, ok := sigIDs[sig]; !ok {
			sigIDs[sig] = int64(len(sigIDs))
		}
		jSig[j] = C.int64_t(sigIDs[sig])
		if job.LastStartTimestamp != nil {
			jLastStart[j] = C.int64_t(job.LastStartTimestamp.UnixNano())
		}
		// pod-sets in name order; the rank is what PodSetOrderFn's name tie-break compares
		psNames := make([]string, 0, len(job.PodSets))
		for name := range job.PodSets {
			psNames = append(psNames, name)
		}
		sort.Strings(psNames)
		jFirstPS[j], jNPS[j] = C.int32_t(si), C.int32_t(len(psNames))
		psIndex := map[string]int{}
		for r, name := range psNames {
			psIndex[name] = si
			psJob[si], psMin[si], psRank[si] = C.int32_t(j), C.int32_t(job.PodSets[name].GetMinAvailable()), C.uint32_t(r)
			si++
		}
		tasks := make([]*pod_info.PodInfo, 0, len(job.GetAllPodsMap()))
		for _, t := range job.GetAllPodsMap() {
			tasks = append(tasks, t)
		}
		sort.Slice(tasks, func(a, b int) bool { return tasks[a].UID < tasks[b].UID })
		jFirstPod[j], jNPods[j] = C.int32_t(pi), C.int32_t(len(tasks))
		for _, t := range tasks {
			p.pods = append(p.pods, t)
			podUIDs = append(podUIDs, string(t.UID))
			req[0*P+pi] = C.double(t.ResReq.Cpu())
			req[1*P+pi] = C.double(t.ResReq.Memory())
			req[2*P+pi] = C.double(t.ResReq.GPUs()) // fractions: the portion rounded to 1/100 (gpu_resource_requirment.go:230-234)
			req[3*P+pi] = 1                          // pods := 1 (api/pod_info/pod_info.go:373-393)
			pJob[pi] = C.int32_t(j)
			pPS[pi] = C.int32_t(psIndex[t.SubGroupName])
			pStatus[pi] = statusBit(t.Status)
			pNode[pi], pNominated[pi], pGroup[pi] = -1, -1, -1
			if ni, ok := nodeIdx[t.NodeName]; ok {
				pNode[pi] = C.int32_t(ni)
			}
			if ni, ok := nodeIdx[t.Pod.Status.NominatedNodeName]; ok { // plugins/nominatednode/nominatednode.go:29-41
				pNominated[pi] = C.int32_t(ni)
			}
			if t.Pod.Spec.SchedulerName != params.schedulerName { // plugins/proportion/proportion.go:276-285
				pFlags[pi] |= C.KAI_POD_FOREIGN_SCHEDULER
			}
			if prio, ok := taskPriority(t); ok { // plugins/taskorder/task_order.go:28-63
				pFlags[pi] |= C.KAI_POD_HAS_TASK_PRIORITY
				pTaskPrio[pi] = C.int32_t(prio)
			}
			pFlags[pi] |= podModelFlags(t)
			if t.ResReq.IsFractionalRequest() && t.ResReq.GetNumOfGpuDevices() == 1 { // ABI v4 / v5: a fraction, or MiB, of ONE device
				if t.IsMemoryRequest() { // pod_info.go:463-468: GPUs() and the portion are 0, the request is the memory
					pGpuMem[pi] = C.int64_t(t.ResReq.GpuMemory())
				} else {
					pPortion[pi] = C.double(t.ResReq.GpuFractionalPortion())
				}
				if len(t.GPUGroups) > 0 {
					pGroup[pi] = C.int32_t(classes.groupID(t.NodeName, t.GPUGroups[0]))
				}
			}
			pCreated[pi] = C.int64_t(t.Pod.CreationTimestamp.UnixNano())
			pClass[pi] = C.int32_t(classes.podClass(t)) // NodeAffinity / nodeSelector / tolerations, canonicalised
			pi++
		}
	}
	copy(pUID, rankStrings(podUIDs))
	for i, n := range p.nodes {
		nodeClass[i] = C.int32_t(classes.nodeClass(n))
	}
	fit := classes.fitTable(p) // [pod classes][node classes], 1 = every static upstream Filter passes (k8s_internal/predicates/predicates.go:70-165)

	s.n_nodes, s.node_allocatable, s.node_flags, s.node_gpu_count, s.node_name_rank, s.node_class = C.int32_t(N), ptr(alloc), ptr(flags), ptr(gpuCount), ptr(cNodeRank), ptr(nodeClass)
	s.n_pods, s.pod_req, s.pod_job, s.pod_podset, s.pod_status, s.pod_node = C.int32_t(P), ptr(req), ptr(pJob), ptr(pPS), ptr(pStatus), ptr(pNode)
	s.pod_flags, s.pod_task_priority, s.pod_created_ns, s.pod_uid_rank, s.pod_class, s.pod_nominated_node = ptr(pFlags), ptr(pTaskPrio), ptr(pCreated), ptr(pUID), ptr(pClass), ptr(pNominated)
	s.n_podsets, s.podset_job, s.podset_min_available, s.podset_name_rank = C.int32_t(S), ptr(psJob), ptr(psMin), ptr(psRank)
	s.n_jobs, s.job_queue, s.job_priority, s.job_preemptible, s.job_created_ns, s.job_uid_rank = C.int32_t(J), ptr(jQueue), ptr(jPrio), ptr(jPreempt), ptr(jCreated), ptr(jUID)
	s.job_first_pod, s.job_n_pods, s.job_first_podset, s.job_n_podsets = ptr(jFirstPod), ptr(jNPods), ptr(jFirstPS), ptr(jNPS)
	s.n_queues, s.queue_parent, s.queue_priority, s.queue_created_ns, s.queue_uid_rank = C.int32_t(Q), ptr(qParent), ptr(qPrio), ptr(qCreated), ptr(qUID)
	s.queue_deserved, s.queue_limit, s.queue_oqw, s.queue_usage = ptr(qDeserved), ptr(qLimit), ptr(qOqw), ptr(qUsage)
	s.n_pod_classes, s.n_node_classes, s.class_fit = C.int32_t(classes.nPod()), C.int32_t(classes.nNode()), ptr(fit)
	s.job_signature, s.job_last_start_ns, s.queue_preempt_min_runtime_ns, s.queue_reclaim_min_runtime_ns = ptr(jSig), ptr(jLastStart), ptr(qPreMR), ptr(qRecMR)
	s.pod_gpu_portion, s.pod_gpu_group, s.node_gpu_memory, s.pod_gpu_memory = ptr(pPortion), ptr(pGroup), ptr(gpuMem), ptr(pGpuMem)
	packTopologies(p, ssn, nodeIdx) // Topology CRs -> node_domain / domain tables; RootSubGroupSet -> group tables (plugins/topology/topology_plugin.go:57-110)
	return p
}

// ------------------------------------------------------------------------------------------------ framework.Plugin
type packParams struct{ schedulerName, gpuWorkerLabel, cpuWorkerLabel string }

type plugin struct {
	params packParams
	pack   *packedSnapshot
	prev   *packedSnapshot // the last cycle's pack, whose session stays open: the next cycle sends a delta against it (kai_session_update_rows)
}

// Now is the cycle's clock (the minruntime plugin's "now"); a test replaces it.
var Now = time.Now

var current *plugin

func New(args framework.PluginArguments) framework.Plugin {
	current = &plugin{params: packParams{schedulerName: args["schedulerName"], gpuWorkerLabel: args["gpuWorkerNodeLabelKey"], cpuWorkerLabel: args["cpuWorkerNodeLabelKey"]}}
	return current
}
func (p *plugin) Name() string { return "gpucore" }
func (p *plugin) OnSessionOpen(ssn *framework.Session) { // framework/interface.go:49-55
	p.pack = packSnapshot(ssn, p.params)
	// The cycle's clock, every cycle, before the session is opened or updated: kai_config.now_ns of Init was only the first cycle's.
	C.kai_core_set_now(core, C.int64_t(Now().UnixNano()))
	// Between two cycles most of the snapshot stays the same: when the new pack differs from the last one only in pod status / node / shared-GPU group,
	// node flags / allocatable, queue rows (quota, limit, over-quota weight, usage, priority, min-runtimes) and the jobs' last start times, the open session
	// takes a delta and the changed rows (cost in proportion to the change) instead of the whole snapshot.
	if p.prev != nil && !p.prev.fallback && sameStructure(p.prev, p.pack) {
		d := packDelta(p.prev, p.pack)
		rc := C.kai_session_update_rows(core, &d.delta, &d.rows)
		d.free()
		if rc == 0 {
			p.dropPrev()
			return
		}
	}
	p.dropPrev()
	if rc := C.kai_session_open(core, &p.pack.soa); rc != 0 {
		p.pack.fallback = true // e.g. KAI_ERR_UNSUPPORTED: leave this cycle to the Go actions
	}
}
func (p *plugin) OnSessionClose(*framework.Session) {
	// the session stays open for the next cycle's delta; kai_session_open / kai_session_update of that cycle replace it
	if p.pack.fallback {
		C.kai_session_close(core)
		p.pack.free()
	} else {
		p.prev = p.pack
	}
	p.pack = nil
}
func (p *plugin) dropPrev() {
	if p.prev != nil {
		p.prev.free()
		p.prev = nil
	}
}

// ------------------------------------------------------------------------------------------------ session delta (kai_session_update_rows)
type packedDelta struct {
	delta  C.kai_session_delta
	rows   C.kai_session_rows
	allocs []unsafe.Pointer
}

func (d *packedDelta) free() {
	for _, a := range d.allocs {
		C.free(a)
	}
	d.allocs = nil
}

func bytesOf[T any](p *T, n int) []byte {
	if p == nil || n <= 0 {
		return nil
	}
	var zero T
	return unsafe.Slice((*byte)(unsafe.Pointer(p)), n*int(unsafe.Sizeof(zero)))
}

// the same snapshot structure: the same counts and every array byte for byte equal, except what the delta carries (pod status / node / shared-GPU group, node
// flags / allocatable) and what the rows carry (queue deserved / limit / oqw / usage / priority / min-runtimes, job last start)
func sameStructure(a, b *packedSnapshot) bool {
	x, y := &a.soa, &b.soa
	if x.n_res != y.n_res || x.n_nodes != y.n_nodes || x.n_pods != y.n_pods || x.n_podsets != y.n_podsets || x.n_jobs != y.n_jobs || x.n_queues != y.n_queues ||
		x.n_pod_classes != y.n_pod_classes || x.n_node_classes != y.n_node_classes || x.n_topologies != y.n_topologies || x.n_topo_levels != y.n_topo_levels ||
		x.n_domains != y.n_domains || x.n_groups != y.n_groups {
		return false
	}
	N, P, S, J, Q, R := int(x.n_nodes), int(x.n_pods), int(x.n_podsets), int(x.n_jobs), int(x.n_queues), int(x.n_res)
	Tn, TL, D, G := int(x.n_topologies), int(x.n_topo_levels), int(x.n_domains), int(x.n_groups)
	eq := func(u, v []byte) bool { return string(u) == string(v) }
	same := eq(bytesOf(x.node_gpu_count, N), bytesOf(y.node_gpu_count, N)) && eq(bytesOf(x.node_name_rank, N), bytesOf(y.node_name_rank, N)) &&
		eq(bytesOf(x.node_class, N), bytesOf(y.node_class, N)) && eq(bytesOf(x.node_gpu_memory, N), bytesOf(y.node_gpu_memory, N)) &&
		eq(bytesOf(x.pod_req, R*P), bytesOf(y.pod_req, R*P)) && eq(bytesOf(x.pod_job, P), bytesOf(y.pod_job, P)) && eq(bytesOf(x.pod_podset, P), bytesOf(y.pod_podset, P)) &&
		eq(bytesOf(x.pod_flags, P), bytesOf(y.pod_flags, P)) && eq(bytesOf(x.pod_task_priority, P), bytesOf(y.pod_task_priority, P)) &&
		eq(bytesOf(x.pod_created_ns, P), bytesOf(y.pod_created_ns, P)) && eq(bytesOf(x.pod_uid_rank, P), bytesOf(y.pod_uid_rank, P)) &&
		eq(bytesOf(x.pod_class, P), bytesOf(y.pod_class, P)) && eq(bytesOf(x.pod_nominated_node, P), bytesOf(y.pod_nominated_node, P)) &&
		eq(bytesOf(x.pod_gpu_portion, P), bytesOf(y.pod_gpu_portion, P)) && eq(bytesOf(x.pod_gpu_memory, P), bytesOf(y.pod_gpu_memory, P)) &&
		eq(bytesOf(x.podset_job, S), bytesOf(y.podset_job, S)) && eq(bytesOf(x.podset_min_available, S), bytesOf(y.podset_min_available, S)) &&
		eq(bytesOf(x.podset_name_rank, S), bytesOf(y.podset_name_rank, S)) &&
		eq(bytesOf(x.job_queue, J), bytesOf(y.job_queue, J)) && eq(bytesOf(x.job_priority, J), bytesOf(y.job_priority, J)) &&
		eq(bytesOf(x.job_preemptible, J), bytesOf(y.job_preemptible, J)) && eq(bytesOf(x.job_created_ns, J), bytesOf(y.job_created_ns, J)) &&
		eq(bytesOf(x.job_uid_rank, J), bytesOf(y.job_uid_rank, J)) && eq(bytesOf(x.job_first_pod, J), bytesOf(y.job_first_pod, J)) &&
		eq(bytesOf(x.job_n_pods, J), bytesOf(y.job_n_pods, J)) && eq(bytesOf(x.job_first_podset, J), bytesOf(y.job_first_podset, J)) &&
		eq(bytesOf(x.job_n_podsets, J), bytesOf(y.job_n_podsets, J)) && eq(bytesOf(x.job_signature, J), bytesOf(y.job_signature, J)) &&
		eq(bytesOf(x.job_root_group, J), bytesOf(y.job_root_group, J)) &&
		eq(bytesOf(x.queue_parent, Q), bytesOf(y.queue_parent, Q)) &&
		eq(bytesOf(x.queue_created_ns, Q), bytesOf(y.queue_created_ns, Q)) && eq(bytesOf(x.queue_uid_rank, Q), bytesOf(y.queue_uid_rank, Q)) &&
		eq(bytesOf(x.class_fit, int(x.n_pod_classes)*int(x.n_node_classes)), bytesOf(y.class_fit, int(y.n_pod_classes)*int(y.n_node_classes))) &&
		eq(bytesOf(x.topo_level_off, Tn+1), bytesOf(y.topo_level_off, Tn+1)) && eq(bytesOf(x.node_domain, TL*N), bytesOf(y.node_domain, TL*N)) &&
		eq(bytesOf(x.domain_level, D), bytesOf(y.domain_level, D)) && eq(bytesOf(x.domain_parent, D), bytesOf(y.domain_parent, D)) && eq(bytesOf(x.domain_id_rank, D), bytesOf(y.domain_id_rank, D)) &&
		eq(bytesOf(x.group_job, G), bytesOf(y.group_job, G)) && eq(bytesOf(x.group_parent, G), bytesOf(y.group_parent, G)) && eq(bytesOf(x.group_name_rank, G), bytesOf(y.group_name_rank, G)) &&
		eq(bytesOf(x.group_topology, G), bytesOf(y.group_topology, G)) && eq(bytesOf(x.group_required_level, G), bytesOf(y.group_required_level, G)) &&
		eq(bytesOf(x.group_preferred_level, G), bytesOf(y.group_preferred_level, G)) &&
		eq(bytesOf(x.podset_group, S), bytesOf(y.podset_group, S)) && eq(bytesOf(x.podset_topology, S), bytesOf(y.podset_topology, S)) &&
		eq(bytesOf(x.podset_required_level, S), bytesOf(y.podset_required_level, S)) && eq(bytesOf(x.podset_preferred_level, S), bytesOf(y.podset_preferred_level, S)) &&
		eq(bytesOf(x.res_mig_gpus, R), bytesOf(y.res_mig_gpus, R)) && eq(bytesOf(x.res_mig_memory, R), bytesOf(y.res_mig_memory, R))
	// an optional array present in one pack and absent in the other is a structural change too (the pod_gpu_group array travels in the delta; an array of the
	// rows may appear, the library then creates it — but it cannot go away again)
	gone := func(u, v unsafe.Pointer) bool { return u != nil && v == nil }
	return same && (x.pod_gpu_portion == nil) == (y.pod_gpu_portion == nil) && (x.pod_gpu_memory == nil) == (y.pod_gpu_memory == nil) &&
		(x.node_gpu_memory == nil) == (y.node_gpu_memory == nil) && (x.job_signature == nil) == (y.job_signature == nil) &&
		!gone(unsafe.Pointer(x.queue_usage), unsafe.Pointer(y.queue_usage)) && !gone(unsafe.Pointer(x.job_last_start_ns), unsafe.Pointer(y.job_last_start_ns)) &&
		!gone(unsafe.Pointer(x.queue_preempt_min_runtime_ns), unsafe.Pointer(y.queue_preempt_min_runtime_ns)) &&
		!gone(unsafe.Pointer(x.queue_reclaim_min_runtime_ns), unsafe.Pointer(y.queue_reclaim_min_runtime_ns))
}

// the pods and nodes whose status / node / group or flags / allocatable differ between the two packs, and the queues and jobs whose rows differ, in C memory
func packDelta(a, b *packedSnapshot) *packedDelta {
	x, y := &a.soa, &b.soa
	N, P, R := int(y.n_nodes), int(y.n_pods), int(y.n_res)
	xs, ys := unsafe.Slice(x.pod_status, P), unsafe.Slice(y.pod_status, P)
	xn, yn := unsafe.Slice(x.pod_node, P), unsafe.Slice(y.pod_node, P)
	group := func(s *C.kai_snapshot_soa, i int) C.int32_t {
		if s.pod_gpu_group == nil {
			return -1
		}
		return unsafe.Slice(s.pod_gpu_group, P)[i]
	}
	var pods []int
	for i := 0; i < P; i++ {
		if xs[i] != ys[i] || xn[i] != yn[i] || group(x, i) != group(y, i) {
			pods = append(pods, i)
		}
	}
	xf, yf := unsafe.Slice(x.node_flags, N), unsafe.Slice(y.node_flags, N)
	xa, ya := unsafe.Slice(x.node_allocatable, R*N), unsafe.Slice(y.node_allocatable, R*N)
	var nodes []int
	for n := 0; n < N; n++ {
		diff := xf[n] != yf[n]
		for r := 0; r < R && !diff; r++ {
			diff = xa[r*N+n] != ya[r*N+n]
		}
		if diff {
			nodes = append(nodes, n)
		}
	}
	d := &packedDelta{}
	alloc := func(bytes int) unsafe.Pointer { m := C.malloc(C.size_t(max(bytes, 1))); d.allocs = append(d.allocs, m); return m }
	np, nn := len(pods), len(nodes)
	pod := unsafe.Slice((*C.int32_t)(alloc(4*np)), max(np, 1))
	st := unsafe.Slice((*C.int32_t)(alloc(4*np)), max(np, 1))
	nd := unsafe.Slice((*C.int32_t)(alloc(4*np)), max(np, 1))
	gr := unsafe.Slice((*C.int32_t)(alloc(4*np)), max(np, 1))
	for k, i := range pods {
		pod[k], st[k], nd[k], gr[k] = C.int32_t(i), ys[i], yn[i], group(y, i)
	}
	node := unsafe.Slice((*C.int32_t)(alloc(4*nn)), max(nn, 1))
	fl := unsafe.Slice((*C.uint32_t)(alloc(4*nn)), max(nn, 1))
	al := unsafe.Slice((*C.double)(alloc(8*R*nn)), max(R*nn, 1))
	for k, n := range nodes {
		node[k], fl[k] = C.int32_t(n), yf[n]
		for r := 0; r < R; r++ {
			al[r*nn+k] = ya[r*N+n]
		}
	}
	d.delta.version = C.KAI_DELTA_VERSION
	d.delta.n_pods, d.delta.pod, d.delta.pod_status, d.delta.pod_node = C.int32_t(np), &pod[0], &st[0], &nd[0]
	if y.pod_gpu_group != nil || x.pod_gpu_group != nil {
		d.delta.pod_gpu_group = &gr[0]
	}
	d.delta.n_nodes, d.delta.node, d.delta.node_flags, d.delta.node_allocatable = C.int32_t(nn), &node[0], &fl[0], &al[0]
	packRows(d, x, y, alloc)
	return d
}

// The queue and job rows that differ (kai_session_rows).  A changed queue sends all of its rows; an optional array the new pack lacks stays NULL (sameStructure
// has made sure the old pack lacked it too), one the old pack lacked reads as the value an absent array stands for.
func packRows(d *packedDelta, x, y *C.kai_snapshot_soa, alloc func(int) unsafe.Pointer) {
	Q, J := int(y.n_queues), int(y.n_jobs)
	f64 := func(p *C.double, n, i int, absent C.double) C.double {
		if p == nil {
			return absent
		}
		return unsafe.Slice(p, n)[i]
	}
	i64 := func(p *C.int64_t, n, i int, absent C.int64_t) C.int64_t {
		if p == nil {
			return absent
		}
		return unsafe.Slice(p, n)[i]
	}
	var queues, jobs []int
	for q := 0; q < Q; q++ {
		diff := unsafe.Slice(x.queue_priority, Q)[q] != unsafe.Slice(y.queue_priority, Q)[q] ||
			i64(x.queue_preempt_min_runtime_ns, Q, q, -1) != i64(y.queue_preempt_min_runtime_ns, Q, q, -1) ||
			i64(x.queue_reclaim_min_runtime_ns, Q, q, -1) != i64(y.queue_reclaim_min_runtime_ns, Q, q, -1)
		for k := 0; k < 3 && !diff; k++ {
			at := k*Q + q
			diff = f64(x.queue_deserved, 3*Q, at, 0) != f64(y.queue_deserved, 3*Q, at, 0) || f64(x.queue_limit, 3*Q, at, 0) != f64(y.queue_limit, 3*Q, at, 0) ||
				f64(x.queue_oqw, 3*Q, at, 0) != f64(y.queue_oqw, 3*Q, at, 0) || f64(x.queue_usage, 3*Q, at, 0) != f64(y.queue_usage, 3*Q, at, 0)
		}
		if diff {
			queues = append(queues, q)
		}
	}
	for j := 0; j < J; j++ {
		if i64(x.job_last_start_ns, J, j, 0) != i64(y.job_last_start_ns, J, j, 0) {
			jobs = append(jobs, j)
		}
	}
	r := &d.rows
	r.version = C.KAI_ROWS_VERSION
	nq, nj := len(queues), len(jobs)
	if nq > 0 {
		qi := unsafe.Slice((*C.int32_t)(alloc(4*nq)), nq)
		pr := unsafe.Slice((*C.int32_t)(alloc(4*nq)), nq)
		quad := [4][]C.double{}
		for a := range quad {
			quad[a] = unsafe.Slice((*C.double)(alloc(8*3*nq)), 3*nq)
		}
		mr := [2][]C.int64_t{unsafe.Slice((*C.int64_t)(alloc(8*nq)), nq), unsafe.Slice((*C.int64_t)(alloc(8*nq)), nq)}
		src := [4]*C.double{y.queue_deserved, y.queue_limit, y.queue_oqw, y.queue_usage}
		for i, q := range queues {
			qi[i], pr[i] = C.int32_t(q), unsafe.Slice(y.queue_priority, Q)[q]
			for a := range quad {
				for k := 0; k < 3; k++ {
					quad[a][k*nq+i] = f64(src[a], 3*Q, k*Q+q, 0)
				}
			}
			mr[0][i], mr[1][i] = i64(y.queue_preempt_min_runtime_ns, Q, q, -1), i64(y.queue_reclaim_min_runtime_ns, Q, q, -1)
		}
		r.n_queues, r.queue, r.queue_priority = C.int32_t(nq), &qi[0], &pr[0]
		r.queue_deserved, r.queue_limit, r.queue_oqw = &quad[0][0], &quad[1][0], &quad[2][0]
		if y.queue_usage != nil {
			r.queue_usage = &quad[3][0]
		}
		if y.queue_preempt_min_runtime_ns != nil {
			r.queue_preempt_min_runtime_ns = &mr[0][0]
		}
		if y.queue_reclaim_min_runtime_ns != nil {
			r.queue_reclaim_min_runtime_ns = &mr[1][0]
		}
	}
	if nj > 0 { // (a differing row means the new pack has the array)
		ji := unsafe.Slice((*C.int32_t)(alloc(4*nj)), nj)
		ls := unsafe.Slice((*C.int64_t)(alloc(8*nj)), nj)
		for i, j := range jobs {
			ji[i], ls[i] = C.int32_t(j), unsafe.Slice(y.job_last_start_ns, J)[j]
		}
		r.n_jobs, r.job, r.job_last_start_ns = C.int32_t(nj), &ji[0], &ls[0]
	}
}

// ------------------------------------------------------------------------------------------------ framework.Action
type action struct {
	kind     C.int
	name     framework.ActionType
	goAction framework.Action // the reference implementation: taken whenever the device path declines
}

func (a *action) Name() framework.ActionType { return a.name }
func (a *action) Execute(ssn *framework.Session) { // framework/interface.go:41-47
	if current == nil || current.pack == nil || current.pack.fallback {
		a.goAction.Execute(ssn)
		return
	}
	if zeroDepth[a.kind] {
		return // queueDepthPerAction 0: every leaf heap stays empty (kai_cgo_config.go), the action tries no job — neither here nor on the device
	}
	pack := current.pack
	capOps := C.int64_t(2*len(pack.pods) + 64)
	ops := (*C.kai_op)(C.malloc(C.size_t(capOps) * C.size_t(unsafe.Sizeof(C.kai_op{}))))
	defer C.free(unsafe.Pointer(ops))
	var n C.int64_t
	if rc := C.kai_action_execute(core, a.kind, ops, capOps, &n); rc != 0 {
		// The device may have applied part of the action before it failed (e.g. KAI_ERR_CAPACITY after some rounds), and in any case it will not see what
		// the Go action does now: the rest of this cycle stays on the Go actions.
		pack.fallback = true
		a.goAction.Execute(ssn)
		return
	}
	if !replay(ssn, a.name, pack, unsafe.Slice(ops, int(n))) {
		pack.fallback = true // the live session and the device state have parted: nothing more from the device in this cycle
	}
}

// BestNodes: Session.OrderedNodesByTask + FittingNode (framework/session.go:201-264) for many tasks against the device's current session state, in ONE
// kai_best_nodes call — what a Go action that stays on the host asks instead of one kai_best_node per task (a gang walked over a SubsetNodesFn result,
// a "why is this pod pending" query over a queue).  nodeSets[i] is the node set of tasks[i] (nil = all nodes); tasks that share a slice (the tasks of one
// job after SubsetNodesFn) share one bitmap row.  Returns per task the node (nil when nothing fits) and whether the placement would be a pipeline.
// ok = false: no device session, a task or node the snapshot does not know, or a refusal — the caller asks the Go session instead.
func BestNodes(tasks []*pod_info.PodInfo, nodeSets [][]*node_info.NodeInfo, pipelineOnly bool) (nodes []*node_info.NodeInfo, isPipeline []bool, ok bool) {
	if current == nil || current.pack == nil || current.pack.fallback || len(nodeSets) != len(tasks) {
		return nil, nil, false
	}
	pack := current.pack
	if len(tasks) == 0 {
		return nil, nil, true
	}
	queries, bitmaps, nRows, known := nodeQueries(pack, tasks, nodeSets, pipelineOnly)
	if !known {
		return nil, nil, false
	}
	// cgo: the arrays hold no Go pointers, so they may be passed for the duration of the call
	answers := make([]C.kai_node_answer, len(tasks))
	if rc := C.kai_best_nodes(core, &queries[0], C.int32_t(len(queries)), ptr(bitmaps), C.int32_t(nRows), &answers[0]); rc != 0 {
		return nil, nil, false
	}
	nodes = make([]*node_info.NodeInfo, len(tasks))
	isPipeline = make([]bool, len(tasks))
	for i, a := range answers {
		if a.node >= 0 {
			nodes[i] = pack.nodes[a.node]
		}
		isPipeline[i] = a.is_pipeline != 0
	}
	return nodes, isPipeline, true
}

// OrderedNodes: per task the first k (1 .. C.KAI_ORDERED_MAX_K) entries of Session.OrderedNodesByTask that pass FittingNode, best first, in ONE kai_ordered_nodes
// call: the list the reference's allocation walks (actions/common/allocate.go), of which BestNodes answers the head.  For a task whose remaining predicates only Go
// can evaluate (KAI_POD_CPU_FALLBACK: inter-pod affinity, host ports, volumes, DRA) the caller runs its filter down nodes[i] and stops at the first pass, instead
// of a Go scan of every node when the one best node fails it; "why is this pod pending" tooling reads the runners-up.  The arguments are BestNodes'.
// nodes[i] holds at most k nodes (fewer: nothing else fits), isPipeline[i][j] belongs to nodes[i][j].  ok = false: as BestNodes, or k out of range.
func OrderedNodes(tasks []*pod_info.PodInfo, nodeSets [][]*node_info.NodeInfo, pipelineOnly bool, k int) (nodes [][]*node_info.NodeInfo, isPipeline [][]bool, ok bool) {
	if current == nil || current.pack == nil || current.pack.fallback || len(nodeSets) != len(tasks) || k < 1 || k > C.KAI_ORDERED_MAX_K {
		return nil, nil, false
	}
	pack := current.pack
	if len(tasks) == 0 {
		return nil, nil, true
	}
	queries, bitmaps, nRows, known := nodeQueries(pack, tasks, nodeSets, pipelineOnly)
	if !known {
		return nil, nil, false
	}
	// cgo: the arrays hold no Go pointers, so they may be passed for the duration of the call
	answers := make([]C.kai_node_answer, len(tasks)*k)
	counts := make([]C.int32_t, len(tasks))
	if rc := C.kai_ordered_nodes(core, &queries[0], C.int32_t(len(queries)), ptr(bitmaps), C.int32_t(nRows), C.int32_t(k), &answers[0], &counts[0]); rc != 0 {
		return nil, nil, false
	}
	nodes = make([][]*node_info.NodeInfo, len(tasks))
	isPipeline = make([][]bool, len(tasks))
	for i := range tasks {
		n := int(counts[i])
		nodes[i] = make([]*node_info.NodeInfo, n)
		isPipeline[i] = make([]bool, n)
		for j := 0; j < n; j++ {
			a := answers[i*k+j]
			nodes[i][j] = pack.nodes[a.node]
			isPipeline[i][j] = a.is_pipeline != 0
		}
	}
	return nodes, isPipeline, true
}

// nodeQueries: what BestNodes and OrderedNodes send — a kai_node_query per task and the node sets as bitmap rows (nRows of them; tasks that share a slice share a
// row).  ok = false: a task or node the snapshot does not know.
func nodeQueries(pack *packedSnapshot, tasks []*pod_info.PodInfo, nodeSets [][]*node_info.NodeInfo, pipelineOnly bool) (queries []C.kai_node_query, bitmaps []C.uint32_t, nRows int, ok bool) {
	podOf := make(map[*pod_info.PodInfo]int, len(pack.pods))
	for i, t := range pack.pods {
		podOf[t] = i
	}
	nodeOf := make(map[*node_info.NodeInfo]int, len(pack.nodes))
	for i, n := range pack.nodes {
		nodeOf[n] = i
	}
	words := (len(pack.nodes) + 31) / 32
	type setKey struct { // slices of one backing array with one length are one node set; every empty set is the same set
		first **node_info.NodeInfo
		n     int
	}
	rows := map[setKey]int{}
	queries = make([]C.kai_node_query, len(tasks))
	for i, t := range tasks {
		p, known := podOf[t]
		if !known {
			return nil, nil, 0, false
		}
		queries[i].pod = C.int32_t(p)
		queries[i].nodeset = -1
		if pipelineOnly {
			queries[i].flags = C.KAI_QUERY_PIPELINE_ONLY
		}
		set := nodeSets[i]
		if set == nil || words == 0 {
			continue
		}
		key := setKey{nil, 0}
		if len(set) > 0 {
			key = setKey{&set[0], len(set)}
		}
		row, seen := rows[key]
		if !seen {
			row = len(bitmaps) / words
			bitmaps = append(bitmaps, make([]C.uint32_t, words)...)
			for _, n := range set {
				ni, known := nodeOf[n]
				if !known {
					return nil, nil, 0, false
				}
				bitmaps[row*words+ni>>5] |= 1 << (uint(ni) & 31)
			}
			rows[key] = row
		}
		queries[i].nodeset = C.int32_t(row)
	}
	if words > 0 {
		nRows = len(bitmaps) / words
	}
	return queries, bitmaps, nRows, true
}

// AppliedOp is one operation a Go-run action committed through a live Statement: what ApplyOps hands to kai_ops_apply.  Stmt numbers the Statements in commit
// order (non-decreasing along the slice); Node is the node of an Allocate / Pipeline, and the node the task is evicted from for an Evict.
type AppliedOp struct {
	Kind int32 // C.KAI_OP_ALLOCATE / KAI_OP_PIPELINE / KAI_OP_EVICT
	Task *pod_info.PodInfo
	Node *node_info.NodeInfo
	Stmt int32
}

// ApplyOps: kai_ops_apply for a wrapper that runs ONE action in Go and wants the device back for the next one: the operations the Go action's Statements
// committed go into the device session, which then is where the live session is.  It is NOT wired into action.Execute below, which still sets `fallback` for the
// rest of the cycle on any non-zero status: a wrapper that calls it has to (1) collect what the Go action's Statements committed, in commit order, and (2) know that
// the device wrote NOTHING for that action — true for a refusal made before the first launch (KAI_ERR_UNSUPPORTED for use_scheduling_signatures without job
// signatures), not for KAI_ERR_CAPACITY or a device fault, after which the device session is somewhere inside the action and there is no undo.
// false: no device session (or `fallback` already set), a task or node the snapshot does not know, or a refusal of kai_ops_apply (an operation whose precondition
// fails against the device state: the two have parted) — `fallback` is set then.
func ApplyOps(applied []AppliedOp) bool {
	if current == nil || current.pack == nil || current.pack.fallback {
		return false
	}
	pack := current.pack
	if len(applied) == 0 {
		return true
	}
	podOf := make(map[*pod_info.PodInfo]int, len(pack.pods))
	for i, t := range pack.pods {
		podOf[t] = i
	}
	nodeOf := make(map[*node_info.NodeInfo]int, len(pack.nodes))
	for i, n := range pack.nodes {
		nodeOf[n] = i
	}
	ops := make([]C.kai_op, len(applied))
	for i, a := range applied {
		p, knownPod := podOf[a.Task]
		n, knownNode := nodeOf[a.Node]
		if !knownPod || !knownNode {
			pack.fallback = true
			return false
		}
		ops[i].seq = C.int64_t(i)
		ops[i].kind = C.int32_t(a.Kind)
		ops[i].pod = C.int32_t(p)
		ops[i].node = C.int32_t(n)
		ops[i].job = -1
		ops[i].stmt = C.int32_t(a.Stmt)
	}
	var res C.kai_apply_result
	if rc := C.kai_ops_apply(core, &ops[0], C.int64_t(len(ops)), 0, &res); rc != 0 {
		pack.fallback = true // the live session and the device state have parted: nothing more from the device in this cycle
		return false
	}
	return true
}

// Statement is the device session's one open (uncommitted) Statement (kai_stmt_*, include/kai_core.h): what a Go-side allocate loop for a job the device cannot
// place itself applies its operations to — Begin, per node set of SubsetNodes a Checkpoint, per task OrderedNodes and Apply, Rollback when the gang does not fit,
// Commit or Discard at the end, as allocateSubGroupSet and attemptToAllocateJob use framework.Statement (actions/common/allocate.go).  Source only: nothing in
// action.Execute below uses it.  While it is open the device's actions, ApplyOps and StaleGangEviction are refused (KAI_ERR_STATE).  Every method returns false
// without a device session, with `fallback` set, for a task or node the snapshot does not know and for a refusal of the entry point; a refused Apply (an
// operation whose precondition fails) leaves the Statement open with its log as it was, so the caller may roll back and go on.
type Statement struct {
	pack   *packedSnapshot
	podOf  map[*pod_info.PodInfo]int
	nodeOf map[*node_info.NodeInfo]int
}

// Begin: kai_stmt_begin on the current device session; nil when there is none or a Statement is open already.
func Begin() *Statement {
	if current == nil || current.pack == nil || current.pack.fallback {
		return nil
	}
	pack := current.pack
	if rc := C.kai_stmt_begin(core, C.KAI_STMT_VERSION); rc != 0 {
		return nil
	}
	s := &Statement{pack: pack, podOf: make(map[*pod_info.PodInfo]int, len(pack.pods)), nodeOf: make(map[*node_info.NodeInfo]int, len(pack.nodes))}
	for i, t := range pack.pods {
		s.podOf[t] = i
	}
	for i, n := range pack.nodes {
		s.nodeOf[n] = i
	}
	return s
}

// Apply: kai_stmt_apply — the operations applied without the commit (an allocated task is left Allocated) and appended to the log.  Stmt of AppliedOp is not read.
func (s *Statement) Apply(applied []AppliedOp) bool {
	if s == nil || current == nil || s.pack != current.pack || s.pack.fallback {
		return false
	}
	if len(applied) == 0 {
		return true
	}
	ops := make([]C.kai_op, len(applied))
	for i, a := range applied {
		p, knownPod := s.podOf[a.Task]
		n, knownNode := s.nodeOf[a.Node]
		if !knownPod || !knownNode {
			return false
		}
		ops[i].seq = C.int64_t(i)
		ops[i].kind = C.int32_t(a.Kind)
		ops[i].pod = C.int32_t(p)
		ops[i].node = C.int32_t(n)
		ops[i].job = -1
	}
	var res C.kai_stmt_result
	return C.kai_stmt_apply(core, &ops[0], C.int64_t(len(ops)), 0, &res) == 0
}

// PlaceGang is one gang of Statement.Place: its tasks in the order they are placed, its node sets as indices into the call's bitmap rows in the order they are tried
// (-1: all nodes), and its row of the call's score rows / deciles (-1: none).  PlacedGang is its answer: whether a set took it, which one (index in Sets, -1), the
// sets tried, per tried set the index of the first task it had no node for (len(Tasks) for the set that took it, -1: not tried), and its operations.
type PlaceGang struct {
	Tasks  []*pod_info.PodInfo
	Sets   []int32
	Scores int32
}
type PlacedGang struct {
	Placed    bool
	Set       int32
	SetsTried int32
	FailAt    []int32
	Ops       []AppliedOp
}

// Place: kai_stmt_place — whole gangs placed on their node sets in one call: per gang a checkpoint, its sets in order, per set its tasks in order, each on the best
// node of the set at the state its predecessors left; a set without a node for a task is rolled back and the next one is tried (allocatePodSet's loop without its
// SubsetNodesFn: bitmaps, scoreRows and deciles are SubsetNodes' outputs).  The Statement stays open; the operations are in its log.  A refusal (a task that is not
// Pending, a task the snapshot does not know) leaves the Statement as it was and returns nil, false.
func (s *Statement) Place(gangs []PlaceGang, bitmaps []uint32, nRows int, scoreRows []C.kai_topo_score_row, deciles []uint8, pipelineOnly bool) ([]PlacedGang, bool) {
	if s == nil || current == nil || s.pack != current.pack || s.pack.fallback {
		return nil, false
	}
	if len(gangs) == 0 {
		return nil, true
	}
	gv := make([]C.kai_place_gang, len(gangs))
	var tasks, sets []C.int32_t
	for g, gang := range gangs {
		gv[g] = C.kai_place_gang{first_task: C.int32_t(len(tasks)), n_tasks: C.int32_t(len(gang.Tasks)), first_set: C.int32_t(len(sets)), n_sets: C.int32_t(len(gang.Sets)), scores: C.int32_t(gang.Scores)}
		for _, t := range gang.Tasks {
			p, known := s.podOf[t]
			if !known {
				return nil, false
			}
			tasks = append(tasks, C.int32_t(p))
		}
		for _, r := range gang.Sets {
			sets = append(sets, C.int32_t(r))
		}
	}
	if len(tasks) == 0 || len(sets) == 0 {
		return nil, false
	}
	params := C.kai_place_params{version: C.KAI_PLACE_VERSION}
	if pipelineOnly {
		params.flags = C.KAI_PLACE_PIPELINE_ONLY
	}
	answers := make([]C.kai_place_answer, len(gangs))
	failAt := make([]C.int32_t, len(sets))
	ops := make([]C.kai_op, len(tasks))
	var rows *C.uint32_t
	if nRows > 0 && len(bitmaps) > 0 {
		rows = (*C.uint32_t)(unsafe.Pointer(&bitmaps[0]))
	}
	var sr *C.kai_topo_score_row
	var dc *C.uint8_t
	if len(scoreRows) > 0 && len(deciles) > 0 {
		sr, dc = &scoreRows[0], (*C.uint8_t)(unsafe.Pointer(&deciles[0]))
	}
	var got C.int64_t
	var res C.kai_stmt_result
	if rc := C.kai_stmt_place(core, &params, &gv[0], C.int32_t(len(gv)), &tasks[0], C.int32_t(len(tasks)), &sets[0], C.int32_t(len(sets)), rows, C.int32_t(nRows),
		sr, dc, C.int32_t(len(scoreRows)), &answers[0], &failAt[0], &ops[0], C.int64_t(len(ops)), &got, &res); rc != 0 {
		if rc == C.KAI_ERR_DEVICE_FAULT {
			s.pack.fallback = true
		}
		return nil, false
	}
	out := make([]PlacedGang, len(gangs))
	for g := range out {
		a := answers[g]
		out[g] = PlacedGang{Placed: a.status == C.KAI_PLACE_PLACED, Set: int32(a.set), SetsTried: int32(a.sets_tried)}
		for i := 0; i < int(gv[g].n_sets); i++ {
			out[g].FailAt = append(out[g].FailAt, int32(failAt[int(gv[g].first_set)+i]))
		}
		for i := int(a.first_op); i < int(a.first_op+a.n_ops); i++ {
			out[g].Ops = append(out[g].Ops, AppliedOp{Kind: int32(ops[i].kind), Task: s.pack.pods[int(ops[i].pod)], Node: s.pack.nodes[int(ops[i].node)]})
		}
	}
	return out, true
}

// Checkpoint: kai_stmt_checkpoint — the log's length (no device call); -1 on a refusal.
func (s *Statement) Checkpoint() int64 {
	var cp C.int64_t
	if s == nil || current == nil || s.pack != current.pack || C.kai_stmt_checkpoint(core, &cp) != 0 {
		return -1
	}
	return int64(cp)
}

// Rollback: kai_stmt_rollback — the operations behind the checkpoint undone, last first.
func (s *Statement) Rollback(cp int64) bool {
	var res C.kai_stmt_result
	return s != nil && current != nil && s.pack == current.pack && C.kai_stmt_rollback(core, C.int64_t(cp), 0, &res) == 0
}

// Discard: kai_stmt_discard — every operation undone, the Statement closed.
func (s *Statement) Discard() bool {
	var res C.kai_stmt_result
	return s != nil && current != nil && s.pack == current.pack && C.kai_stmt_discard(core, 0, &res) == 0
}

// Commit: kai_stmt_commit — the surviving operations committed on the device (allocated tasks become Binding) and handed back in log order, for the caller to replay
// into the live session as action.Execute replays an action's; the Statement is closed.  A device fault sets `fallback`.
func (s *Statement) Commit() ([]AppliedOp, bool) {
	if s == nil || current == nil || s.pack != current.pack || s.pack.fallback {
		return nil, false
	}
	n := s.Checkpoint()
	if n < 0 {
		return nil, false
	}
	ops := make([]C.kai_op, n+1)
	var got C.int64_t
	var res C.kai_stmt_result
	if rc := C.kai_stmt_commit(core, &ops[0], C.int64_t(n), &got, &res); rc != 0 {
		if rc == C.KAI_ERR_DEVICE_FAULT {
			s.pack.fallback = true
		}
		return nil, false
	}
	out := make([]AppliedOp, int(got))
	for i := range out {
		out[i] = AppliedOp{Kind: int32(ops[i].kind), Task: s.pack.pods[int(ops[i].pod)], Node: s.pack.nodes[int(ops[i].node)]}
	}
	return out, true
}

// StaleGangEviction: the stalegangeviction action (actions/stalegangeviction/stalegangeviction.go:29-90) decided by the device against ITS session state — where
// the placement actions of this cycle left it — in ONE kai_stale_gang_eviction call.  StalenessInfo.TimeStamp of every job goes down as nanoseconds (0 = nil), the
// clock is the handle's (kai_core_set_now; OnSessionOpen sets it from Now), gracePeriod is ssn.GetGlobalDefaultStalenessGracePeriod() (negative: never evict).
// What comes back is replayed into the live session: each run of equal kai_op.stmt is one job's gang, evicted task by task through ssn.Evict (which is
// ssn.Cache.Evict plus the session's own bookkeeping, framework/session.go:127-150) with EvictionGangSize = the run's length and Action = StaleGangEviction, as the
// reference does without a Statement; then TimeStamp / Stale are written back to every job.  The device keeps nanoseconds; the annotation the status updater
// writes from TimeStamp keeps seconds (RFC 3339, cache/status_updater/default_status_updater.go:446-456), so a stamp read back from the pod group in the next
// cycle is up to a second older than the one set here — the same truncation the Go action lives with.
// An eviction the live session refuses is logged by the reference and skipped; here it also sets `fallback`, because the device has evicted the task.
// false: no device session (or `fallback` already set), or a refusal of the entry point (shared-GPU requests, a clock that is not above 0): nothing was written,
// the caller runs the Go action instead.
func StaleGangEviction(ssn *framework.Session, gracePeriod time.Duration) bool {
	if current == nil || current.pack == nil || current.pack.fallback {
		return false
	}
	pack := current.pack
	if len(pack.jobs) == 0 {
		return true
	}
	since := make([]C.int64_t, len(pack.jobs))
	for j, job := range pack.jobs {
		if job.StalenessInfo.TimeStamp != nil {
			since[j] = C.int64_t(job.StalenessInfo.TimeStamp.UnixNano())
		}
	}
	stale := make([]C.uint8_t, len(pack.jobs))
	capOps := len(pack.pods) // always suffices
	ops := make([]C.kai_op, capOps+1)
	params := C.kai_stale_params{version: C.KAI_STALE_VERSION, grace_ns: C.int64_t(gracePeriod.Nanoseconds())}
	var n C.int64_t
	var res C.kai_stale_result
	// cgo: the arrays hold no Go pointers, so they may be passed for the duration of the call
	if rc := C.kai_stale_gang_eviction(core, &params, &since[0], &stale[0], &ops[0], C.int64_t(capOps), &n, &res); rc != 0 {
		return false // decided before the first write: the device session and the caller's arrays are as they were
	}
	ok := true
	for i := 0; i < int(n); {
		id, first := ops[i].stmt, i
		for i < int(n) && ops[i].stmt == id {
			i++
		}
		job := pack.jobs[ops[first].job]
		meta := eviction_info.EvictionMetadata{EvictionGangSize: i - first, Action: string(framework.StaleGangEviction)}
		for k := first; k < i; k++ {
			task := pack.pods[ops[k].pod]
			if err := ssn.Evict(task, api.GetGangEvictionMessage(task, job), meta); err != nil {
				ok = false // the live session and the device state have parted: nothing more from the device in this cycle
			}
		}
	}
	for j, job := range pack.jobs {
		if since[j] == 0 {
			job.StalenessInfo.TimeStamp, job.StalenessInfo.Stale = nil, false
			continue
		}
		if job.StalenessInfo.TimeStamp == nil || job.StalenessInfo.TimeStamp.UnixNano() != int64(since[j]) {
			t := time.Unix(0, int64(since[j]))
			job.StalenessInfo.TimeStamp = &t
		}
		if stale[j] != 0 {
			job.StalenessInfo.Stale = true
		}
	}
	if !ok {
		pack.fallback = true
	}
	return true
}

// JobOrder: what the reflectjoborder plugin computes in OnSessionOpen (plugins/reflectjoborder/reflect_job_order.go:41-66) — the PopNextJob sequence of a
// JobsOrderByQueues with FilterNonPending, FilterUnready and the allocate action's queue depth — decided by the device against ITS session state in ONE
// kai_job_order call, in the plugin's own document shape (GlobalOrder, QueueOrder with id and priority).  depth 0 takes kai_config.queue_depth[allocate], which
// OnSessionOpen packed from ssn.GetJobsDepth(framework.Allocate).  The call changes nothing on the device, so it may be made at any point of the cycle: in front of
// the first action it answers what the plugin answers, behind an action where the queue stands now.  Not registered anywhere: a deployment that serves
// /get-job-order from the device session calls it from its handler.
// nil: no device session (or `fallback` already set), or a refusal of the entry point: the caller builds the order in Go.
func JobOrder() *reflectjoborder.ReflectJobOrder {
	if current == nil || current.pack == nil || current.pack.fallback {
		return nil
	}
	pack := current.pack
	doc := &reflectjoborder.ReflectJobOrder{GlobalOrder: make([]reflectjoborder.JobOrder, 0), QueueOrder: make(map[common_info.QueueID][]reflectjoborder.JobOrder)}
	if len(pack.jobs) == 0 {
		return doc
	}
	order := make([]C.int32_t, len(pack.jobs)) // n_jobs always suffices
	params := C.kai_job_order_params{version: C.KAI_JOB_ORDER_VERSION}
	var n C.int32_t
	// cgo: the array holds no Go pointers, so it may be passed for the duration of the call
	if rc := C.kai_job_order(core, &params, &order[0], C.int32_t(len(order)), &n, nil, nil, nil); rc != 0 {
		return nil
	}
	for i := 0; i < int(n); i++ {
		job := pack.jobs[order[i]]
		jo := reflectjoborder.JobOrder{ID: job.UID, Priority: job.Priority}
		doc.GlobalOrder = append(doc.GlobalOrder, jo)
		doc.QueueOrder[job.Queue] = append(doc.QueueOrder[job.Queue], jo) // pop order filtered by the leaf queue: what job_queue_pos_out indexes
	}
	return doc
}

// SubsetNodes: the SubsetNodesFn of the default tier — the topology plugin's subSetNodesFn (plugins/topology/job_filtering.go:34-112) — for the root sub-group
// sets of many jobs over all nodes, decided by the device against ITS session state in ONE kai_subset_nodes call (two where the first guess of the capacity is too
// small: the call then says how many sets there are).  sets[i] are the node sets of jobs[i] in the order the allocate action tries them, as BestNodes /
// OrderedNodes take them for nodeSets; no set: the job cannot be placed under its constraint now (status[i] says why: C.KAI_SUBSET_NO_TOPOLOGY, _NO_FIT,
// _BAD_LEVEL).  The composed walk of a topology gang whose pods only Go can filter (KAI_POD_CPU_FALLBACK): SubsetNodes, then per node set OrderedNodes for the
// gang's tasks and the Go filter down each list — no pass over the nodes on the host.  The call changes nothing on the device; the preferred-level node scores
// are not part of the answer.  Inner sub-groups and pod-sets are asked through the C call with a node set's row as the parent row.  Not registered anywhere.
// ok = false: no device session (or `fallback` already set), a job the snapshot does not know, or a refusal of the entry point: the caller asks the Go session.
func SubsetNodes(jobs []*podgroup_info.PodGroupInfo) (sets [][][]*node_info.NodeInfo, status []int, ok bool) {
	if current == nil || current.pack == nil || current.pack.fallback {
		return nil, nil, false
	}
	pack := current.pack
	if len(jobs) == 0 {
		return nil, nil, true
	}
	jobOf := make(map[*podgroup_info.PodGroupInfo]int, len(pack.jobs))
	for i, j := range pack.jobs {
		jobOf[j] = i
	}
	queries := make([]C.kai_subset_query, len(jobs))
	for i, j := range jobs {
		idx, known := jobOf[j]
		if !known {
			return nil, nil, false
		}
		queries[i] = C.kai_subset_query{job: C.int32_t(idx), group: -1, podset: -1, nodeset: -1}
	}
	words := (len(pack.nodes) + 31) / 32
	params := C.kai_subset_params{version: C.KAI_SUBSET_VERSION}
	answers := make([]C.kai_subset_answer, len(jobs))
	capSets := 8*len(jobs) + 64
	var records []C.kai_node_set
	var rows []C.uint32_t
	var n C.int64_t
	for try := 0; ; try++ {
		records = make([]C.kai_node_set, capSets+1)
		rows = make([]C.uint32_t, capSets*words+1)
		// cgo: the arrays hold no Go pointers, so they may be passed for the duration of the call
		rc := C.kai_subset_nodes(core, &params, &queries[0], C.int32_t(len(queries)), nil, 0, &answers[0], &records[0], C.int64_t(capSets), &n, &rows[0], nil)
		if rc == C.KAI_ERR_CAPACITY && try == 0 {
			capSets = int(n) // decided before the first write: the arrays are as they were
			continue
		}
		if rc != 0 {
			return nil, nil, false
		}
		break
	}
	sets = make([][][]*node_info.NodeInfo, len(jobs))
	status = make([]int, len(jobs))
	for i, a := range answers {
		status[i] = int(a.status)
		sets[i] = make([][]*node_info.NodeInfo, int(a.n_sets))
		for k := 0; k < int(a.n_sets); k++ {
			r := int(a.first) + k
			set := make([]*node_info.NodeInfo, 0, int(records[r].n_nodes))
			for w := 0; w < words; w++ {
				for bits := uint32(rows[r*words+w]); bits != 0; bits &= bits - 1 {
					set = append(set, pack.nodes[w*32+mathbits.TrailingZeros32(bits)])
				}
			}
			sets[i][k] = set
		}
	}
	return sets, status, true
}

// SubsetNodesScored: SubsetNodes with the topology plugin's node scores (calculateNodeScores, plugins/topology/node_scoring.go:37-53) in ONE kai_subset_nodes_scored call.
// scores[i] is what OrderedNodesScored takes for the tasks of jobs[i]: the row of the job's root sub-group set — nil where the reference records none (no preferred level,
// no constraint, a common domain that cannot take the gang): such a task is ordered without a topology term, or, for an inner sub-group asked through the C call, with the
// nearest ancestor's row that is not KAI_TOPO_SCORES_NONE.  The scores are computed once per sub-group and NOT again between the tasks of a gang, as in the reference.
// Not registered anywhere.  ok = false: as SubsetNodes.
type TopologyScores struct {
	row     C.kai_topo_score_row
	deciles []C.uint8_t // [n_domains]: floor((idx + 1) / n * 10) per scored domain, KAI_TOPO_NO_SCORE elsewhere
}

func SubsetNodesScored(jobs []*podgroup_info.PodGroupInfo) (sets [][][]*node_info.NodeInfo, scores []*TopologyScores, status []int, ok bool) {
	if current == nil || current.pack == nil || current.pack.fallback {
		return nil, nil, nil, false
	}
	pack := current.pack
	if len(jobs) == 0 {
		return nil, nil, nil, true
	}
	jobOf := make(map[*podgroup_info.PodGroupInfo]int, len(pack.jobs))
	for i, j := range pack.jobs {
		jobOf[j] = i
	}
	queries := make([]C.kai_subset_query, len(jobs))
	for i, j := range jobs {
		idx, known := jobOf[j]
		if !known {
			return nil, nil, nil, false
		}
		queries[i] = C.kai_subset_query{job: C.int32_t(idx), group: -1, podset: -1, nodeset: -1}
	}
	words := (len(pack.nodes) + 31) / 32
	domains := int(pack.soa.n_domains)
	params := C.kai_subset_params{version: C.KAI_SUBSET_VERSION}
	answers := make([]C.kai_subset_answer, len(jobs))
	scoreRows := make([]C.kai_topo_score_row, len(jobs))
	deciles := make([]C.uint8_t, len(jobs)*domains+1)
	capSets := 8*len(jobs) + 64
	var records []C.kai_node_set
	var rows []C.uint32_t
	var n C.int64_t
	for try := 0; ; try++ {
		records = make([]C.kai_node_set, capSets+1)
		rows = make([]C.uint32_t, capSets*words+1)
		// cgo: the arrays hold no Go pointers, so they may be passed for the duration of the call
		rc := C.kai_subset_nodes_scored(core, &params, &queries[0], C.int32_t(len(queries)), nil, 0, &answers[0], &records[0], C.int64_t(capSets), &n, &rows[0], &scoreRows[0], &deciles[0], nil)
		if rc == C.KAI_ERR_CAPACITY && try == 0 {
			capSets = int(n) // decided before the first write: the arrays are as they were
			continue
		}
		if rc != 0 {
			return nil, nil, nil, false
		}
		break
	}
	sets = make([][][]*node_info.NodeInfo, len(jobs))
	scores = make([]*TopologyScores, len(jobs))
	status = make([]int, len(jobs))
	for i, a := range answers {
		status[i] = int(a.status)
		sets[i] = make([][]*node_info.NodeInfo, int(a.n_sets))
		for k := 0; k < int(a.n_sets); k++ {
			r := int(a.first) + k
			set := make([]*node_info.NodeInfo, 0, int(records[r].n_nodes))
			for w := 0; w < words; w++ {
				for bits := uint32(rows[r*words+w]); bits != 0; bits &= bits - 1 {
					set = append(set, pack.nodes[w*32+mathbits.TrailingZeros32(bits)])
				}
			}
			sets[i][k] = set
		}
		if scoreRows[i].level_row != C.KAI_TOPO_SCORES_NONE {
			scores[i] = &TopologyScores{row: scoreRows[i], deciles: deciles[i*domains : (i+1)*domains : (i+1)*domains]}
		}
	}
	return sets, scores, status, true
}

// OrderedNodesScored: OrderedNodes with the topology plugin's term (nodeOrderFn, plugins/topology/node_scoring.go:17-35) in ONE kai_ordered_nodes_scored call:
// scores[i] (of SubsetNodesScored; nil = none) is the row task i is scored with — a node whose domain has no score in it is dropped from the list, the others get
// decile x scores.Topology on top.  With k = 1 it is the scored BestNodes.  Not registered anywhere.  ok = false: as OrderedNodes, or len(scores) != len(tasks).
func OrderedNodesScored(tasks []*pod_info.PodInfo, nodeSets [][]*node_info.NodeInfo, scores []*TopologyScores, pipelineOnly bool, k int) (nodes [][]*node_info.NodeInfo, isPipeline [][]bool, ok bool) {
	if current == nil || current.pack == nil || current.pack.fallback || len(nodeSets) != len(tasks) || len(scores) != len(tasks) || k < 1 || k > C.KAI_ORDERED_MAX_K {
		return nil, nil, false
	}
	pack := current.pack
	if len(tasks) == 0 {
		return nil, nil, true
	}
	plain, bitmaps, nRows, known := nodeQueries(pack, tasks, nodeSets, pipelineOnly)
	if !known {
		return nil, nil, false
	}
	domains := int(pack.soa.n_domains)
	rowOf := map[*TopologyScores]int{} // tasks that share a TopologyScores share a row
	var scoreRows []C.kai_topo_score_row
	var deciles []C.uint8_t
	queries := make([]C.kai_scored_query, len(tasks))
	for i, q := range plain {
		queries[i] = C.kai_scored_query{pod: q.pod, nodeset: q.nodeset, flags: q.flags, scores: -1}
		sc := scores[i]
		if sc == nil {
			continue
		}
		row, seen := rowOf[sc]
		if !seen {
			if len(sc.deciles) != domains {
				return nil, nil, false
			}
			row = len(scoreRows)
			rowOf[sc] = row
			scoreRows = append(scoreRows, sc.row)
			deciles = append(deciles, sc.deciles...)
		}
		queries[i].scores = C.int32_t(row)
	}
	deciles = append(deciles, 0) // (never empty: &deciles[0] below)
	scoreRows = append(scoreRows, C.kai_topo_score_row{level_row: C.KAI_TOPO_SCORES_NONE})
	// cgo: the arrays hold no Go pointers, so they may be passed for the duration of the call
	answers := make([]C.kai_node_answer, len(tasks)*k)
	counts := make([]C.int32_t, len(tasks))
	if rc := C.kai_ordered_nodes_scored(core, &queries[0], C.int32_t(len(queries)), ptr(bitmaps), C.int32_t(nRows), &scoreRows[0], &deciles[0], C.int32_t(len(scoreRows)-1), C.int32_t(k), &answers[0], &counts[0]); rc != 0 {
		return nil, nil, false
	}
	nodes = make([][]*node_info.NodeInfo, len(tasks))
	isPipeline = make([][]bool, len(tasks))
	for i := range tasks {
		n := int(counts[i])
		nodes[i] = make([]*node_info.NodeInfo, n)
		isPipeline[i] = make([]bool, n)
		for j := 0; j < n; j++ {
			a := answers[i*k+j]
			nodes[i][j] = pack.nodes[a.node]
			isPipeline[i][j] = a.is_pipeline != 0
		}
	}
	return nodes, isPipeline, true
}

// replay: the committed operations through the real Statement.  kai_op.stmt numbers the Statements of the action in
// commit order; one id = one Statement, e.g. a reclaim "evict A, evict B, pipeline C" (framework/statement.go:536-575).
// An operation the live session refuses (the cache moved on since the snapshot, a bind conflict) discards its whole Statement —
// a gang is committed entirely or not at all — and ends the replay: false.
func replay(ssn *framework.Session, action framework.ActionType, pack *packedSnapshot, ops []C.kai_op) bool {
	groups := carray[C.int32_t](pack, len(pack.pods)) // PodInfo.GPUGroups[0] of the fraction pods after the action (freed with the snapshot)
	haveGroups := len(pack.pods) > 0 && C.kai_pod_gpu_groups(core, ptr(groups), C.int(len(pack.pods))) == 0
	for i := 0; i < len(ops); {
		stmt := ssn.Statement()
		id := ops[i].stmt
		var err error
		// EvictionMetadata of the Statement's evictions (actions/common/action.go:34-38): the gang = every task the solution evicts, the preemptor = the job the
		// Statement pipelines / allocates.  A Statement of a victim action holds one solution: "evict ..., pipeline the preemptor's tasks" (framework/statement.go:536-575).
		meta := eviction_info.EvictionMetadata{Action: string(action)}
		// The jobs re-placed behind the evictions are the victims' jobs AND the preemptor, in job order (actions/common/action.go:65-122), so the first pipelined task can be
		// a victim's: the preemptor is the job of a placed task that was Pending when the Statement began and that this Statement does not evict.
		// An elastic victim job may also place a pod of its own that was Pending in the same Statement (it is re-placed like any job of the scenario), and it can sort in front
		// of the preemptor: the preemptor is a job NONE of whose pods this Statement evicts.
		var preemptor *podgroup_info.PodGroupInfo
		evicted := map[C.int32_t]bool{}
		victimJob := map[common_info.PodGroupID]bool{}
		for k := i; k < len(ops) && ops[k].stmt == id; k++ {
			if ops[k].kind == C.KAI_OP_EVICT {
				meta.EvictionGangSize++
				evicted[ops[k].pod] = true
				victimJob[pack.pods[ops[k].pod].Job] = true
			}
		}
		for k := i; k < len(ops) && ops[k].stmt == id && preemptor == nil; k++ {
			task := pack.pods[ops[k].pod]
			if (ops[k].kind == C.KAI_OP_ALLOCATE || ops[k].kind == C.KAI_OP_PIPELINE) && !evicted[ops[k].pod] && !victimJob[task.Job] && task.Status == pod_status.Pending {
				preemptor = ssn.ClusterInfo.PodGroupInfos[task.Job]
			}
		}
		messages := map[int]string{} // getEvictionMessages: every message from the state BEFORE the first eviction (actions/common/action.go:51-60)
		if preemptor != nil {
			meta.Preemptor = &types.NamespacedName{Namespace: preemptor.Namespace, Name: preemptor.Name}
			for k := i; k < len(ops) && ops[k].stmt == id; k++ {
				if ops[k].kind == C.KAI_OP_EVICT {
					messages[k] = utils.GetMessageOfEviction(ssn, action, pack.pods[ops[k].pod], preemptor)
				}
			}
		}
		for ; i < len(ops) && ops[i].stmt == id; i++ {
			if err != nil {
				continue // skip the rest of a Statement that is going to be discarded
			}
			task := pack.pods[ops[i].pod]
			switch ops[i].kind {
			case C.KAI_OP_ALLOCATE, C.KAI_OP_PIPELINE:
				node := pack.nodes[ops[i].node]
				if haveGroups && task.IsSharedGPURequest() && groups[ops[i].pod] >= 0 {
					// SelectedGPUGroups of the BindRequest (cache/cache.go:290-330) come from PodInfo.GPUGroups: the group the device chose
					task.GPUGroups = []string{pack.classes.groupName(node.Name, int32(groups[ops[i].pod]))}
				}
				if ops[i].kind == C.KAI_OP_ALLOCATE {
					err = stmt.Allocate(task, node.Name)
				} else {
					err = stmt.Pipeline(task, node.Name, task.Status != pod_status.Pending)
				}
			case C.KAI_OP_EVICT:
				err = stmt.Evict(task, messages[i], meta)
			}
		}
		if err != nil {
			stmt.Discard()
			return false
		}
		if err = stmt.Commit(); err != nil {
			return false
		}
	}
	return true
}

func init() {
	framework.RegisterPluginBuilder("gpucore", New) // framework/plugins.go:31-47
	// framework/plugins.go:49-54: an action registered under the name of the original takes its place in the configured `actions:` list
	framework.RegisterAction(&action{kind: C.KAI_ACTION_ALLOCATE, name: framework.Allocate, goAction: allocate.New()})
	framework.RegisterAction(&action{kind: C.KAI_ACTION_CONSOLIDATION, name: framework.Consolidation, goAction: consolidation.New()})
	framework.RegisterAction(&action{kind: C.KAI_ACTION_RECLAIM, name: framework.Reclaim, goAction: reclaim.New()})
	framework.RegisterAction(&action{kind: C.KAI_ACTION_PREEMPT, name: framework.Preempt, goAction: preempt.New()})
}

// taskPriority, newStaticClasses (podClass / nodeClass / fitTable / groupID / groupName) and packTopologies: kai_cgo_classes.go.
