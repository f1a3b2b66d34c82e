"""kai_stale_gang_eviction without a GPU.

 - the export, the ABI structs and constants, the header text;
 - arguments and call order under the host-only library (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp, as tests/test_ops_apply.py does): every
   host-decidable refusal is made before the first device call and leaves the device memory image, the session and both caller arrays as they were; a warm call allocates neither
   device nor pinned memory.  The kernels of the host-only library do nothing, so what comes back is what was sent: no stale job, no eviction.  KAI_ERR_CAPACITY depends on the
   kernels' count: it is asserted on the emulated kernels, through the same sg_drive the library runs;
 - the kernel bodies and the call's control flow (kai_stale_gangs.hpp) run with emulated lanes by tests/host_sim/stale_gangs_sim.cpp on a session of the host simulation: the
   reference's six cases, a fuzz against the numpy restatement of the rules (tests/stale_gangs_ref.py) and against a twin session that takes the same operations through
   kai_ops_apply's emulated apply, with workgroups of 256, 100 and 1 lanes and with the wave order reversed.
The parity claim on the device is tests/test_gpu_stale_gangs.py."""
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
import stale_gangs_ref as R
from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = T.abi
S = abi.POD_STATUS
WIDE, ENGINE = abi.APPLY_PATH_WIDE, abi.APPLY_PATH_ENGINE
OP_DT = R.OP_DT


def test_exports_and_struct_sizes():
    assert "kai_stale_gang_eviction" in T.pkg.core.EXPORTS
    Pm, Rs = abi.KaiStaleParams, abi.KaiStaleResult
    assert C.sizeof(Pm) == 16 and [f[0] for f in Pm._fields_] == ["version", "flags", "grace_ns"]
    assert (Pm.version.offset, Pm.flags.offset, Pm.grace_ns.offset) == (0, 4, 8)
    assert C.sizeof(Rs) == 24 and [f[0] for f in Rs._fields_] == ["stale_jobs", "expired_jobs", "n_ops", "path", "pad"]
    assert (Rs.stale_jobs.offset, Rs.expired_jobs.offset, Rs.n_ops.offset, Rs.path.offset, Rs.pad.offset) == (0, 4, 8, 16, 20)
    assert (abi.STALE_VERSION, abi.STALE_DRY_RUN) == (1, 1)
    hdr = open(os.path.join(ROOT, "include", "kai_core.h")).read()
    assert "#define KAI_ABI_VERSION 5u" in hdr and abi.KAI_ABI_VERSION == 5, "no existing struct changed: the ABI version stays"
    for text in ("#define KAI_STALE_VERSION 1u", "#define KAI_STALE_DRY_RUN 0x1u", "int kai_stale_gang_eviction(kai_core* core, const kai_stale_params* params,",
                 "typedef struct kai_stale_params { uint32_t version; uint32_t flags; int64_t grace_ns; /* < 0: never evict */ } kai_stale_params;",
                 "typedef struct kai_stale_result { int32_t stale_jobs; int32_t expired_jobs; int64_t n_ops; int32_t path; int32_t pad; } kai_stale_result;"):
        assert text in hdr, text
    assert hasattr(T.pkg.load_library(), "kai_stale_gang_eviction")
    assert hasattr(T.pkg.core.Session, "stale_gang_eviction")


# ---------------------------------------------------------------------------------------------- the host side under the host-only library
DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
Op, Pm, Rs = abi.KaiOp, abi.KaiStaleParams, abi.KaiStaleResult
lib.kai_stale_gang_eviction.argtypes = [C.c_void_p, C.POINTER(Pm), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(Op), C.c_int64, C.POINTER(C.c_int64), C.POINTER(Rs)]
lib.kai_core_set_now.argtypes = [C.c_void_p, C.c_int64]
snap, cfg, _ = pkg.synth.config(1, 0.3)
cfg = abi.copy_config(cfg); cfg.now_ns = 5000
P, J = snap.n_pods, snap.n_jobs
def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]
def call(h, version=1, flags=0, grace=60, since=None, cap=None, null=()):
    """-> [status, the caller's arrays and n_ops untouched]"""
    since = np.full(J, 7, np.int64) if since is None else np.array(since, np.int64)
    since0 = since.copy(); stale = np.full(J, 9, np.uint8); ops = np.zeros(max(P, 1), pkg.core._OP_DTYPE); ops["pad"] = 5
    n = C.c_int64(-3); r = Rs(11, 12, 13, 14, 15); pm = Pm(version, flags, grace)
    rc = lib.kai_stale_gang_eviction(h, None if "params" in null else C.byref(pm), None if "since" in null else since.ctypes.data_as(C.POINTER(C.c_int64)),
                                     None if "stale" in null else stale.ctypes.data_as(C.POINTER(C.c_uint8)), None if "ops" in null else ops.ctypes.data_as(C.POINTER(Op)),
                                     P if cap is None else cap, None if "n_ops" in null else C.byref(n), None if "result" in null else C.byref(r))
    untouched = bool((since == since0).all() and (stale == 9).all() and (ops["pad"] == 5).all() and n.value == -3 and (r.stale_jobs, r.expired_jobs, r.n_ops, r.path, r.pad) == (11, 12, 13, 14, 15))
    return [rc, untouched, n.value, [r.stale_jobs, r.expired_jobs, r.n_ops, r.path, r.pad], bool((since == 0).all()), bool((stale == 0).all())]
res = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
res["before_open"] = call(h)
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = image()
bad = {}
bad["version"] = call(h, version=2)
bad["unknown_flags"] = call(h, flags=2)
bad["unknown_flags_high"] = call(h, flags=0x80000001)
bad["null_params"] = call(h, null=("params",))
bad["null_since"] = call(h, null=("since",))
bad["null_n_ops"] = call(h, null=("n_ops",))
bad["null_ops_with_capacity"] = call(h, null=("ops",))
bad["negative_capacity"] = call(h, cap=-1)
neg = np.full(J, 7, np.int64); neg[J // 2] = -1
bad["negative_since"] = call(h, since=neg)
res["image_unchanged"] = image() == img0
assert lib.kai_core_set_now(h, 0) == 0  # (an upload of its own)
img0 = image()
bad["clock_zero"] = call(h)
res["image_unchanged_clock"] = image() == img0
assert lib.kai_core_set_now(h, 5000) == 0
img0 = image()
res["bad"] = bad
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
res["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
# good calls: what each costs on the device (the kernels of the host-only library do nothing: the counts that come back are the zeros that were sent)
res["good1"] = call(h); i1 = image()
res["good2"] = call(h); i2 = image()
res["null_optional"] = call(h, null=("stale", "result", "ops"), cap=0); i3 = image()
res["dry"] = call(h, flags=1); i4 = image()
res["first_call"] = dict(allocations=i1[1] - img0[1], launches=i1[3] - img0[3], h2d=i1[4] - img0[4], memsets=i1[7] - img0[7], pinned=i1[8] - img0[8])
res["warm_call"] = dict(allocations=i2[1] - i1[1], live_bytes=i2[2] - i1[2], launches=i2[3] - i1[3], h2d=i2[4] - i1[4], h2d_bytes=i2[5] - i1[5], d2d=i2[6] - i1[6], memsets=i2[7] - i1[7], pinned=i2[8] - i1[8])
res["null_optional_call"] = dict(allocations=i3[1] - i2[1], live_bytes=i3[2] - i2[2], launches=i3[3] - i2[3], h2d=i3[4] - i2[4], pinned=i3[8] - i2[8])
res["dry_call"] = dict(allocations=i4[1] - i3[1], live_bytes=i4[2] - i3[2], launches=i4[3] - i3[3], h2d=i4[4] - i3[4], pinned=i4[8] - i3[8])
res["J"] = J
lib.kai_core_destroy(h)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 2, None, C.byref(h2)) == 0
res["sharded"] = call(h2)
lib.kai_core_destroy(h2)
# a session with shared-GPU requests
snap3, cfg3, _ = pkg.synth.config(1, 0.2); pkg.synth.add_fractions(snap3, 7, frac=0.3)
cfg3 = abi.copy_config(cfg3); cfg3.now_ns = 5000
P, J = snap3.n_pods, snap3.n_jobs
h3 = C.c_void_p(); st3 = snap3.as_struct()
assert lib.kai_core_create(C.byref(cfg3), 1, None, C.byref(h3)) == 0 and lib.kai_session_open(h3, C.byref(st3)) == 0
img3 = image()
res["shared"] = call(h3); res["shared_image_unchanged"] = image() == img3
lib.kai_core_destroy(h3)
print(json.dumps(res))
'''


def test_arguments_and_call_order(fake_lib):
    code = f"ROOT = {ROOT!r}\nLIB = {fake_lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["before_open"][:2] == [-6, True], "KAI_ERR_STATE without an open session"
    for k, v in out["bad"].items():
        assert v[:2] == [-1, True], (k, v)
    assert out["image_unchanged"] and out["image_unchanged_clock"], "a refused call allocated or wrote device memory"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["sharded"][:2] == [-5, True], "KAI_ERR_UNSUPPORTED on a handle of a sharded group"
    assert out["shared"][:2] == [-5, True] and out["shared_image_unchanged"], "KAI_ERR_UNSUPPORTED in a session with shared-GPU requests, before the first device call"
    # a call that goes through: nothing is stale for kernels that do nothing — KAI_OK, no operation, the result written, the arrays as the device scratch holds them
    for k in ("good1", "good2", "dry"):
        assert out[k][0] == 0 and out[k][2] == 0 and out[k][3] == [0, 0, 0, abi.APPLY_PATH_NONE, 0], (k, out[k])
    assert out["null_optional"][0] == 0 and out["null_optional"][2] == 0, "job_stale_out, result and (with no capacity) ops_out may be NULL"
    # the device side: one upload (the counts and the timestamps); the Succeeded pass, the job pass, the first-pod pass, the totals and their scan — no emit and no apply launch
    # where nothing is evicted; the first call of a handle also allocates its scratch (zeroed once) and its staging
    assert out["first_call"] == dict(allocations=1, launches=5, h2d=1, memsets=1, pinned=out["first_call"]["pinned"]) and out["first_call"]["pinned"] > 0
    w = out["warm_call"]
    assert w == dict(allocations=0, live_bytes=0, launches=5, h2d=1, h2d_bytes=64 + 8 * out["J"], d2d=0, memsets=0, pinned=0), w
    assert out["null_optional_call"] == dict(allocations=0, live_bytes=0, launches=5, h2d=1, pinned=0)
    assert out["dry_call"] == dict(allocations=0, live_bytes=0, launches=5, h2d=1, pinned=0)


# ---------------------------------------------------------------------------------------------- the kernel bodies with emulated lanes
SIM_SRC = os.path.join(ROOT, "tests", "host_sim", "stale_gangs_sim.cpp")


def sim_lib():
    so = os.path.join(ROOT, "tests", "host_sim", "libstalegangssim.so")
    deps = [SIM_SRC, os.path.join(ROOT, "tests", "host_sim", "sim_session.hpp"), os.path.join(ROOT, "tests", "host_sim", "native_bucket_fill.hpp")] + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    lib = C.CDLL(so)
    lib.kai_sgsim_run.restype = C.c_int
    return lib


def sim_run(snap, cfg, since=None, grace=0, twin_ops=None, dry_run=False, lanes=256, cap=None, pre=(), post=(), no_batch=True):
    """the call (twin_ops None) or the twin's kai_ops_apply of twin_ops, between the actions `pre` and `post` of the host simulation.
    -> Result: status, result fields, ops (kai_op records), since, stale, mid (state right behind the call), and the cycle's operations / final state."""
    lib = sim_lib()
    s = snap.as_struct()
    P, Q, N, J = snap.n_pods, snap.n_queues, snap.n_nodes, snap.n_jobs
    ai = lambda names: (C.c_int * max(len(names), 1))(*[abi.ACTIONS[a] for a in names])
    mode = 0 if twin_ops is None else 1
    since = np.zeros(J, np.int64) if since is None else np.array(since, np.int64)
    stale = np.full(J, 9, np.uint8)
    call_cap = P if cap is None else cap
    sg = np.zeros(max(P, 1), OP_DT); n_sg = C.c_int64(0)
    if mode == 1:
        sg[: len(twin_ops)] = twin_ops; n_sg = C.c_int64(len(twin_ops))
    capo = max(64, 8 * P)
    ops = (abi.KaiOp * capo)(); n_ops = C.c_int64(0)
    status = np.zeros(P, np.int32); node = np.zeros(P, np.int32); mstatus = np.zeros(P, np.int32); mnode = np.zeros(P, np.int32)
    sh_mid = (abi.KaiQueueShare * max(Q, 1))(); sh_fin = (abi.KaiQueueShare * max(Q, 1))(); nd_mid = (abi.KaiNodeState * max(N, 1))(); nd_fin = (abi.KaiNodeState * max(N, 1))()
    hidden = np.zeros(4 * P + 4 * snap.n_podsets + 8 * J + 8, np.int32); n_hidden = C.c_int64(0)
    rc_call = C.c_int(99); res = abi.KaiStaleResult()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    had = os.environ.get("KAI_HOSTSIM_NO_BATCH")
    if no_batch: os.environ["KAI_HOSTSIM_NO_BATCH"] = "1"
    try:
        rc = lib.kai_sgsim_run(C.byref(cfg), C.byref(s), ai(pre), len(pre), C.c_int(mode), since.ctypes.data_as(C.POINTER(C.c_int64)), stale.ctypes.data_as(C.POINTER(C.c_uint8)),
                               C.c_int64(grace), C.c_uint32(abi.STALE_DRY_RUN if dry_run else 0), C.c_int(lanes), C.c_int64(call_cap), sg.ctypes.data_as(C.POINTER(abi.KaiOp)), C.byref(n_sg),
                               C.byref(res), C.byref(rc_call), ai(post), len(post), ip(mstatus), ip(mnode), sh_mid, nd_mid, ip(hidden), C.c_int64(len(hidden)), C.byref(n_hidden),
                               ops, C.c_int64(capo), C.byref(n_ops), ip(status), ip(node), sh_fin, nd_fin)
    finally:
        if no_batch and had is None: del os.environ["KAI_HOSTSIM_NO_BATCH"]
    assert rc == 0, f"kai_sgsim_run rc={rc}"
    mid = T.Result(pod_status=mstatus, pod_node=mnode, shares=T.shares_to_np(sh_mid, Q), nodes=T.nodes_to_np(nd_mid, N, snap.n_res), hidden=hidden[: n_hidden.value].copy())
    return T.Result(status=rc_call.value, stale_jobs=res.stale_jobs, expired_jobs=res.expired_jobs, n_ops=res.n_ops, path=res.path, needed=n_sg.value,
                    sg_ops=sg[: n_sg.value if rc_call.value == 0 else 0].copy(), since=since, stale=stale, mid=mid,
                    ops=[(o.kind, o.pod, o.node, o.job) for o in ops[: n_ops.value]], pod_status=status, pod_node=node, shares_final=T.shares_to_np(sh_fin, Q),
                    nodes=T.nodes_to_np(nd_fin, N, snap.n_res))


def same_mid(a, b, what=""):
    assert (a.mid.pod_status == b.mid.pod_status).all(), f"{what}: pod status, pods {np.nonzero(a.mid.pod_status != b.mid.pod_status)[0][:8].tolist()}"
    assert (a.mid.pod_node == b.mid.pod_node).all(), f"{what}: pod node"
    for k in b.mid.nodes: assert np.array_equal(a.mid.nodes[k], b.mid.nodes[k]), f"{what}: node {k}"
    for k in b.mid.shares: assert np.array_equal(a.mid.shares[k], b.mid.shares[k]), f"{what}: share {k}"
    assert np.array_equal(a.mid.hidden, b.mid.hidden), f"{what}: the state no read-back shows differs at words {np.nonzero(a.mid.hidden != b.mid.hidden)[0][:8].tolist()}"


def against_reference(r, ref, what=""):
    assert r.status == 0, (what, r.status)
    assert np.array_equal(r.since, ref.since), f"{what}: timestamps, jobs {np.nonzero(r.since != ref.since)[0][:8].tolist()}"
    assert np.array_equal(r.stale, ref.expired.astype(np.uint8)), f"{what}: Stale, jobs {np.nonzero(r.stale != ref.expired)[0][:8].tolist()}"
    assert (r.stale_jobs, r.expired_jobs, r.n_ops) == (ref.stale_jobs, ref.expired_jobs, len(ref.ops)), (what, r.stale_jobs, r.expired_jobs, r.n_ops, ref.stale_jobs, ref.expired_jobs, len(ref.ops))
    assert len(r.sg_ops) == len(ref.ops)
    for f in ("seq", "kind", "pod", "node", "job", "stmt", "pad"):
        assert np.array_equal(r.sg_ops[f], ref.ops[f]), f"{what}: operations differ in {f} at {np.nonzero(r.sg_ops[f] != ref.ops[f])[0][:8].tolist()}"


@pytest.fixture(scope="module")
def reference_cases():
    return R.fixture_cases()


def test_the_fixture_covers_the_six_reference_cases(reference_cases):
    assert len(reference_cases) == 6
    assert [c[5] for c in reference_cases] == [0, 0, 1, 0, 3, 0] and {c[4] for c in reference_cases} == {60 * R.SEC}
    assert sorted({int(x) for c in reference_cases for x in R.NOW - c[3][c[3] != 0]}) == [R.SEC, 61 * R.SEC], "StaleDuration"
    assert [c[1].podset_min_available.tolist() for c in reference_cases] == [[1], [2], [2], [1], [2, 1], [2, 1]], "MinAvailable and sub-groups"


@pytest.mark.parametrize("lanes", [256, 100, 1])
@pytest.mark.parametrize("i", range(6))
def test_reference_cases_through_the_emulated_kernels(reference_cases, i, lanes):
    """actions/stalegangeviction/stalegangeviction_test.go: final pod statuses and nodes (TaskExpectedResults) and the number of evictions (NumberOfCacheEvictions)"""
    line, snap, cfg, since, grace, evictions, meta = reference_cases[i]
    r = sim_run(snap, cfg, since, grace, lanes=lanes)
    assert r.status == 0 and r.n_ops == evictions == len(r.sg_ops), (line, r.status, r.n_ops)
    errs = T.check_expectations(snap, meta, r.mid.pod_status, r.mid.pod_node, None)
    assert not errs, (line, errs)
    against_reference(r, R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, grace), f"case at line {line}")
    if evictions: assert len(set(r.sg_ops["stmt"])) == 1, "one job: one EvictionGangSize"


# ---- fuzz: 64 nodes, about 20 000 pods in 5 000 jobs — more than 64 workgroups of 256 lanes, so k_sg_scan's wavefronts hand sums to one another (at 100 lanes and at 1 lane it
# also walks several tiles with a carry)
SEEDS = list(range(20))
NEEDED = ("expired_with_evictions", "stale_inside_grace", "newly_stale", "kept_by_succeeded", "expired_only_releasing", "stale_through_one_podset", "recovered")


@pytest.fixture(scope="module")
def fuzz_cases():
    return {}


def fuzz_case(cache, seed):
    if seed not in cache:
        cache.clear()  # (one snapshot at a time: the seeds come in order)
        cache[seed] = R.fuzz_snapshot(seed)
    return cache[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_against_the_numpy_reference(fuzz_cases, seed):
    """Every seed runs under each grace period of {-1, 0, 60 s} (the timestamps are drawn around that period's limit).  A negative period never evicts, so the two kinds of
    expired jobs are asserted to occur at 0 and at 60 s and asserted NOT to occur at -1; the five other kinds occur at every period."""
    snap, cfg = fuzz_case(fuzz_cases, seed)
    P, J = snap.n_pods, snap.n_jobs
    assert snap.n_nodes == 64 and 18000 <= P <= 24000 and J == 5000 and (P + 255) // 256 > 64
    assert (np.diff(snap.job_first_pod) < 0).any() and (snap.job_n_pods == 0).sum() >= 100 and set(snap.job_n_podsets.tolist()) == {1, 2, 3, 4}
    assert ((snap.job_first_pod // 256) != ((snap.job_first_pod + np.maximum(snap.job_n_pods, 1) - 1) // 256)).sum() >= 10, "jobs that straddle a workgroup boundary"
    assert set(snap.pod_status.tolist()) == set(S.values()), "every status occurs"
    lanes = (256, 100, 1)[seed % 3] if seed >= 3 else 256
    for grace in R.GRACES:
        since = R.fuzz_since(snap, seed, grace)
        assert set(since.tolist()) == {0, R.NOW - grace - 1, R.NOW - grace, R.NOW - grace + 1}
        cat = R.categories(snap, snap.pod_status, since, R.NOW, grace)
        for k in NEEDED:
            if grace < 0 and k.startswith("expired"): assert cat[k] == 0, (seed, grace, k)
            else: assert cat[k] >= 1, (seed, grace, cat)
        ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, grace)
        r = sim_run(snap, cfg, since, grace, lanes=lanes)
        against_reference(r, ref, f"seed {seed} grace {grace} lanes {lanes}")
        assert r.path == (abi.APPLY_PATH_NONE if not len(ref.ops) else ENGINE), "Pipelined pods among the evicted: the engine walk"
        if grace == 0:  # the twin: the same operations through kai_ops_apply's emulated apply
            twin = sim_run(snap, cfg, twin_ops=r.sg_ops, lanes=lanes)
            assert twin.status == 0 and twin.path == r.path
            same_mid(r, twin, f"seed {seed}")
            dry = sim_run(snap, cfg, since, grace, lanes=lanes, dry_run=True)
            against_reference(dry, ref, f"seed {seed} dry run")
            untouched = sim_run(snap, cfg, twin_ops=np.zeros(0, OP_DT))
            same_mid(dry, untouched, f"seed {seed} dry run")
            assert dry.path == r.path


def test_capacity_reports_the_count_and_writes_nothing():
    snap, cfg = R.fuzz_snapshot(3, n_jobs=600)
    since = R.fuzz_since(snap, 3, 0)
    ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, 0)
    assert len(ref.ops) > 1
    untouched = sim_run(snap, cfg, twin_ops=np.zeros(0, OP_DT))
    for cap in (0, len(ref.ops) - 1):
        r = sim_run(snap, cfg, since, 0, cap=cap)
        assert r.status == -4 and r.needed == len(ref.ops)
        assert np.array_equal(r.since, since) and (r.stale == 9).all(), "the caller's arrays"
        same_mid(r, untouched, "capacity")
    r = sim_run(snap, cfg, since, 0, cap=len(ref.ops))
    against_reference(r, ref, "a capacity of exactly the evictions")


def test_wide_path_and_the_next_allocate():
    """no Pipelined pod: the chip-wide apply; the allocate action behind the call commits what it commits behind the twin's kai_ops_apply"""
    snap, cfg = R.fuzz_snapshot(5, n_jobs=600, pipelined=False)
    since = R.fuzz_since(snap, 5, 0)
    ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, 0)
    first = None
    for lanes in (256, 100, 1):
        r = sim_run(snap, cfg, since, 0, lanes=lanes, post=("allocate",))
        against_reference(r, ref, f"{lanes} lanes")
        assert r.path == WIDE and len(ref.ops) > 100
        twin = sim_run(snap, cfg, twin_ops=r.sg_ops, lanes=lanes, post=("allocate",))
        assert twin.path == WIDE
        same_mid(r, twin, f"{lanes} lanes")
        assert r.ops == twin.ops and len(r.ops) > 0, "the next allocate"
        assert (r.pod_status == twin.pod_status).all() and (r.pod_node == twin.pod_node).all()
        first = first or r
        same_mid(r, first, f"{lanes} lanes against 256")


REVERSED = r'''
import json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import test_stale_gangs as t
R = t.R
out = {}
for name, pipelined in (("engine", True), ("wide", False)):
    snap, cfg = R.fuzz_snapshot(11, n_jobs=1500, pipelined=pipelined)
    since = R.fuzz_since(snap, 11, 0)
    ref = R.decide(snap, snap.pod_status, snap.pod_node, since, R.NOW, 0)
    r = t.sim_run(snap, cfg, since, 0)
    t.against_reference(r, ref, name)
    twin = t.sim_run(snap, cfg, twin_ops=r.sg_ops)
    t.same_mid(r, twin, name)
    out[name] = [r.status, r.path, int(r.n_ops)]
print(json.dumps(out))
'''


def test_kernel_bodies_with_the_wave_order_reversed():
    """the emulator's waves take their turns in reverse (KW_EMU_ORDER=1, read once per process: a fresh one): a scan that leaned on the waves' order would differ"""
    sim_lib()  # built before the child starts
    env = dict(os.environ, KW_EMU_ORDER="1")
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + REVERSED], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["engine"][:2] == [0, ENGINE] and got["wide"][:2] == [0, WIDE] and got["engine"][2] > 256 and got["wide"][2] > 256, got


def test_stand_alone_program(tmp_path):
    """the fixed case behind -DKAI_SGSIM_MAIN builds and passes: 256 / 100 / 1 lanes, the twin, a dry run, a capacity refusal, both apply paths; reversed waves too"""
    exe = str(tmp_path / "stale_gangs_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKAI_SGSIM_MAIN", "-o", exe, SIM_SRC])
    for order in ("0", "1"):
        r = subprocess.run([exe], env=dict(os.environ, KW_EMU_ORDER=order), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "stale_gangs_sim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _sanitizer_runtimes(tmp_path):
    """whether the host compiler links and runs a program with -fsanitize=address,undefined"""
    src = tmp_path / "probe.cpp"; src.write_text("int main() { return 0; }\n")
    exe = str(tmp_path / "probe")
    if shutil.which("g++") is None: return "g++ not available"
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, str(src)], capture_output=True, text=True)
    if b.returncode != 0: return "the host compiler has no AddressSanitizer / UBSan runtime: " + b.stderr.strip().splitlines()[-1][:200]
    r = subprocess.run([exe], capture_output=True, text=True)
    return None if r.returncode == 0 else "a program built with -fsanitize=address,undefined does not start here: " + (r.stderr.strip().splitlines() or ["?"])[-1][:200]


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined and run as its own process (nothing sanitized is loaded into Python)"""
    why = _sanitizer_runtimes(tmp_path)
    if why: pytest.skip(why)
    exe = str(tmp_path / "stale_gangs_sim_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKAI_SGSIM_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "stale_gangs_sim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
