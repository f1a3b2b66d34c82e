"""kai_session_update_rows / kai_core_set_now without a GPU: the library's host side (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp,
as tests/test_session_update.py does) checks the arguments of both parts and the call order before anything is written: a valid delta with bad rows leaves the
session's device memory as it was and the session open.  abi.apply_rows builds the snapshot S' and the configuration cfg' a fresh handle opens."""
import json
import os
import subprocess
import sys

import numpy as np

import kai_testlib as T
from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT + "/tests"); sys.path.insert(0, ROOT)
import numpy as np
import kai_testlib as T
pkg = T.pkg; abi = pkg.abi
lib = C.CDLL(LIB)
lib.kai_last_error.restype = C.c_char_p; lib.kai_last_error.argtypes = [C.c_void_p]
lib.kai_core_set_now.argtypes = [C.c_void_p, C.c_int64]
snap, cfg, _ = pkg.synth.config(1, 0.3)
P, N, Q, J = snap.n_pods, snap.n_nodes, snap.n_queues, snap.n_jobs
out = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
good_delta = dict(pods=[0], status=[1], node=[-1])
def upd(delta=None, **rows):
    keep = []
    d = r = None
    if delta is not None:
        d, k = pkg.core.delta_struct(**delta); keep.append(k)
    if rows.pop("with_rows", True):
        r, k = pkg.core.rows_struct(**rows); keep.append(k)
    return lib.kai_session_update_rows(h, None if d is None else C.byref(d), None if r is None else C.byref(r))
out["before_open"] = upd(queues=[0], queue_priority=[1])
out["set_now_before_open"] = lib.kai_core_set_now(h, 5)
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = (C.c_uint64 * 9)(); lib.fakehip_image(img0)
bad = {}
bad["wrong_version"] = upd(good_delta, queues=[0], queue_priority=[1], version=2)
bad["unknown_fields"] = upd(good_delta, fields=0x2)
bad["queue_out_of_range"] = upd(good_delta, queues=[Q], queue_priority=[1])
bad["queue_negative"] = upd(good_delta, queues=[-1], queue_priority=[1])
bad["queue_twice"] = upd(good_delta, queues=[0, 0], queue_priority=[1, 1])
bad["job_out_of_range"] = upd(good_delta, jobs=[J], job_last_start_ns=[1])
bad["job_negative"] = upd(good_delta, jobs=[-1], job_last_start_ns=[1])
bad["job_twice"] = upd(good_delta, jobs=[1, 1], job_last_start_ns=[1, 1])
r, keep = pkg.core.rows_struct(queues=[0], queue_priority=[1]); r.n_queues = -1
bad["negative_queue_count"] = lib.kai_session_update_rows(h, None, C.byref(r))
r, keep = pkg.core.rows_struct(jobs=[0], job_last_start_ns=[1]); r.n_jobs = -1
bad["negative_job_count"] = lib.kai_session_update_rows(h, None, C.byref(r))
r, keep = pkg.core.rows_struct(queues=[0], queue_priority=[1]); r.queue = None
bad["null_queue_index"] = lib.kai_session_update_rows(h, None, C.byref(r))
r, keep = pkg.core.rows_struct(jobs=[0], job_last_start_ns=[1]); r.job = None
bad["null_job_index"] = lib.kai_session_update_rows(h, None, C.byref(r))
# the delta's own refusals still hold through the new entry point, good rows beside them
bad["bad_delta_good_rows"] = upd(dict(pods=[P], status=[1], node=[-1]), queues=[0], queue_priority=[1])
bad["bad_delta_version"] = upd(dict(pods=[0], status=[1], node=[-1], version=2), queues=[0], queue_priority=[1])
out["bad"] = bad
img1 = (C.c_uint64 * 9)(); lib.fakehip_image(img1)
out["image_unchanged"] = list(img0) == list(img1)
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
out["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
out["null_null"] = lib.kai_session_update_rows(h, None, None)
out["empty_rows"] = upd()
out["empty_both"] = upd(dict(pods=[], status=[], node=[]))
out["set_now_open"] = lib.kai_core_set_now(h, 7)
# kai_session_update(d) as before: a NULL delta and a wrong version refused, an empty delta applied
out["update_null"] = lib.kai_session_update(h, None)
d, keep = pkg.core.delta_struct([0], [1], [-1], version=2); out["update_version_2"] = lib.kai_session_update(h, C.byref(d))
d, keep = pkg.core.delta_struct([], [], []); out["update_empty"] = lib.kai_session_update(h, C.byref(d))
# rows of every kind, with a delta, applied
out["all_rows"] = upd(good_delta, now_ns=11, queues=[0, Q - 1], queue_deserved=np.ones((3, 2)), queue_limit=-np.ones((3, 2)), queue_oqw=np.ones((3, 2)), queue_usage=np.zeros((3, 2)),
                      queue_priority=[3, 4], queue_preempt_min_runtime_ns=[-1, 0], queue_reclaim_min_runtime_ns=[5, -1], jobs=[0, J - 1], job_last_start_ns=[1, 2])
out["still_open_after"] = lib.kai_pod_states(h, st_out, nd_out, P)
lib.kai_core_destroy(h)
# S', cfg' from the helper: a snapshot and a configuration a fresh handle opens
s2, c2 = abi.apply_rows(snap, cfg, now_ns=11, queues=[0, Q - 1], queue_usage=np.full((3, 2), 0.5), queue_preempt_min_runtime_ns=[-1, 0], jobs=[0, J - 1], job_last_start_ns=[1, 2])
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(c2), 1, None, C.byref(h2)) == 0
st2 = s2.as_struct()
out["open_s2"] = lib.kai_session_open(h2, C.byref(st2))
lib.kai_core_destroy(h2)
print(json.dumps(out))
'''


def _run(lib):
    code = f"ROOT = {ROOT!r}\nLIB = {lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_rows_arguments_and_call_order(fake_lib):
    out = _run(fake_lib)
    assert out["before_open"] == -6, "KAI_ERR_STATE without an open session"
    assert out["set_now_before_open"] == 0, "kai_core_set_now works without a session"
    for k, rc in out["bad"].items():
        assert rc == -1, (k, rc)
    assert out["image_unchanged"], "a refused call (a valid delta with bad rows among them) wrote to the session's device memory"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["null_null"] == 0 and out["empty_rows"] == 0 and out["empty_both"] == 0
    assert out["set_now_open"] == 0
    assert out["update_null"] == -1 and out["update_version_2"] == -1 and out["update_empty"] == 0, "kai_session_update changed"
    assert out["all_rows"] == 0 and out["still_open_after"] == 0
    assert out["open_s2"] == 0, "kai_session_open refused the snapshot apply_rows built"


def test_exports_declare_rows():
    core = T.pkg.core
    assert "kai_session_update_rows" in core.EXPORTS and "kai_core_set_now" in core.EXPORTS
    lib = T.pkg.load_library()
    assert hasattr(lib, "kai_session_update_rows") and hasattr(lib, "kai_core_set_now")
    assert T.pkg.abi.STATUS_TEXT[-9] == "out of host memory"
    assert T.pkg.abi.ROWS_VERSION == 1


def test_rows_struct_layout():
    """KaiSessionRows against the C struct of include/kai_core.h (LP64): offsets as the compiler lays them out."""
    R = T.pkg.abi.KaiSessionRows
    want = dict(version=0, fields=4, now_ns=8, n_queues=16, queue=24, queue_deserved=32, queue_limit=40, queue_oqw=48, queue_usage=56, queue_priority=64,
                queue_preempt_min_runtime_ns=72, queue_reclaim_min_runtime_ns=80, n_jobs=88, job=96, job_last_start_ns=104)
    assert {k: getattr(R, k).offset for k in want} == want
    import ctypes as C
    assert C.sizeof(R) == 112


def test_apply_rows_builds_the_new_snapshot():
    abi = T.pkg.abi
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    Q, J = snap.n_queues, snap.n_jobs
    assert Q >= 3 and J >= 3 and "job_last_start_ns" not in snap.arrays and "queue_preempt_min_runtime_ns" not in snap.arrays
    qs, js = [0, Q - 1], [1, J - 1]
    des = np.array([[1.0, 2.0], [3.0, -1.0], [5.0, 6.0]])
    before = {k: v.copy() for k, v in snap.arrays.items()}
    now0 = cfg.now_ns
    s2, c2 = abi.apply_rows(snap, cfg, now_ns=now0 + 17, queues=qs, queue_deserved=des, queue_usage=np.full((3, 2), 0.25), queue_priority=[7, 9],
                            queue_preempt_min_runtime_ns=[0, 600], jobs=js, job_last_start_ns=[11, 13])
    assert c2.now_ns == now0 + 17 and cfg.now_ns == now0, "cfg' carries the clock, the original configuration is untouched"
    assert bytes(c2)[:abi.KaiConfig.now_ns.offset] == bytes(cfg)[:abi.KaiConfig.now_ns.offset]
    assert np.array_equal(s2.queue_deserved[:, qs], des) and np.array_equal(s2.queue_usage[:, qs], np.full((3, 2), 0.25))
    assert list(s2.queue_priority[qs]) == [7, 9]
    others_q = np.setdiff1d(np.arange(Q), qs); others_j = np.setdiff1d(np.arange(J), js)
    assert np.array_equal(s2.queue_deserved[:, others_q], snap.queue_deserved[:, others_q]) and np.array_equal(s2.queue_priority[others_q], snap.queue_priority[others_q])
    # arrays the snapshot lacked appear, with the value an absent array stands for in every other row; the one no row names stays absent
    assert list(s2.queue_preempt_min_runtime_ns[qs]) == [0, 600] and (s2.queue_preempt_min_runtime_ns[others_q] == -1).all()
    assert list(s2.job_last_start_ns[js]) == [11, 13] and (s2.job_last_start_ns[others_j] == 0).all()
    assert "queue_reclaim_min_runtime_ns" not in s2.arrays
    assert s2.queue_preempt_min_runtime_ns.dtype == np.int64 and s2.job_last_start_ns.dtype == np.int64
    # the original is untouched, S' packs into the ABI struct, the arrays no row touches are shared
    for k, v in before.items():
        assert np.array_equal(snap.arrays[k], v), k
    assert set(snap.arrays) == set(before)
    s2.as_struct()
    for k in snap.arrays:
        if k not in ("queue_deserved", "queue_usage", "queue_priority"):
            assert s2.arrays[k] is snap.arrays[k], k
    # nothing named: the same snapshot, a copy of the configuration
    s3, c3 = abi.apply_rows(snap, cfg)
    assert all(s3.arrays[k] is snap.arrays[k] for k in snap.arrays) and bytes(c3) == bytes(cfg)
    # index arrays without rows create nothing
    s4, _ = abi.apply_rows(snap, cfg, queues=[], queue_reclaim_min_runtime_ns=[], jobs=[], job_last_start_ns=[])
    assert "job_last_start_ns" not in s4.arrays and "queue_reclaim_min_runtime_ns" not in s4.arrays
