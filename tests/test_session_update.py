"""kai_session_update without a GPU: the library's host side (kai_core.hip compiled host-only and linked with tests/host_sim/fake_hip.cpp, as
tests/test_open_uploads.py does: device memory is host memory, kernels do nothing) checks the delta's arguments and the call order before anything is
written, and a refusal leaves the session open and unchanged.  The delta helper (abi.apply_delta) builds the snapshot S' that kai_session_open accepts.
What an update computes is not checked here (the gather returns nothing under the stand-in runtime): tests/test_update_chains.py checks the chains of updates in
tests/update_chains.py as inputs, tests/test_gpu_update_chains.py walks them on the MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

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
snap, cfg, _ = pkg.synth.config(1, 0.3)
P, N = snap.n_pods, snap.n_nodes
out = {}
h = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h)) == 0
def upd(*a, **kw):
    d, keep = pkg.core.delta_struct(*a, **kw)
    return lib.kai_session_update(h, C.byref(d))
out["before_open"] = upd([0], [1], [-1])
out["null_delta"] = lib.kai_session_update(h, None)
st = snap.as_struct()
assert lib.kai_session_open(h, C.byref(st)) == 0
img0 = (C.c_uint64 * 9)(); lib.fakehip_image(img0)
out["pod_out_of_range"] = upd([P], [1], [-1])
out["pod_negative"] = upd([-1], [1], [-1])
out["node_out_of_range"] = upd([0], [64], [N])
out["node_below_minus_one"] = upd([0], [64], [-2])
out["pod_twice"] = upd([0, 0], [1, 1], [-1, -1])
out["delta_node_out_of_range"] = upd([], [], [], nodes=[N])
out["delta_node_twice"] = upd([], [], [], nodes=[1, 1])
out["wrong_version"] = upd([0], [1], [-1], version=2)
d, keep = pkg.core.delta_struct([0], [1], [-1]); d.pod_status = None
out["null_required"] = lib.kai_session_update(h, C.byref(d))
d, keep = pkg.core.delta_struct([], [], [], nodes=[0]); d.node = None
out["null_node"] = lib.kai_session_update(h, C.byref(d))
img1 = (C.c_uint64 * 9)(); lib.fakehip_image(img1)
out["image_unchanged"] = list(img0) == list(img1)
st_out = (C.c_int32 * P)(); nd_out = (C.c_int32 * P)()
out["still_open"] = lib.kai_pod_states(h, st_out, nd_out, P)
out["empty_delta"] = upd([], [], [])
lib.kai_core_destroy(h)
# S' from the delta helper is a snapshot kai_session_open accepts (placed pods, a cordoned node with new allocatable)
pend = np.nonzero(snap.pod_status == 1)[0][:5]
s2 = abi.apply_delta(snap, pend, [64] * len(pend), [1] * len(pend), None, [0, 3], [0x1, 0x0], snap.node_allocatable[:, [0, 3]] * 2)
h2 = C.c_void_p()
assert lib.kai_core_create(C.byref(cfg), 1, None, C.byref(h2)) == 0
st2 = s2.as_struct()
out["open_s2"] = lib.kai_session_open(h2, C.byref(st2))
out["update_after_open_s2"] = (lambda d: lib.kai_session_update(h2, C.byref(d[0])))(pkg.core.delta_struct([int(pend[0])], [1], [-1]))
lib.kai_core_destroy(h2)
print(json.dumps(out))
'''


def _run(lib):
    code = f"ROOT = {ROOT!r}\nLIB = {lib!r}\n" + DRIVER
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_update_arguments_and_call_order(fake_lib):
    out = _run(fake_lib)
    assert out["before_open"] == -6, "KAI_ERR_STATE without an open session"
    assert out["null_delta"] == -1
    for k in ("pod_out_of_range", "pod_negative", "node_out_of_range", "node_below_minus_one", "pod_twice", "delta_node_out_of_range", "delta_node_twice",
              "wrong_version", "null_required", "null_node"):
        assert out[k] == -1, (k, out[k])
    assert out["image_unchanged"], "a refused delta wrote to the session's device memory"
    assert out["still_open"] == 0, "a refusal closed the session"
    assert out["empty_delta"] == 0
    assert out["open_s2"] == 0, "kai_session_open refused the snapshot the delta helper built"
    assert out["update_after_open_s2"] == 0


def test_exports_declare_update():
    assert "kai_session_update" in T.pkg.core.EXPORTS
    lib = T.pkg.load_library()
    assert hasattr(lib, "kai_session_update")


def test_apply_delta_builds_the_new_snapshot():
    abi = T.pkg.abi
    snap, cfg, _ = T.pkg.synth.config(1, 0.3)
    pend = np.nonzero(snap.pod_status == 1)[0][:3]
    nodes = [0, 2]
    alloc = snap.node_allocatable[:, nodes] * 2
    s2 = abi.apply_delta(snap, pend, [64] * len(pend), [1] * len(pend), [5] * len(pend), nodes, [0x1, 0x0], alloc)
    assert (s2.pod_status[pend] == 64).all() and (s2.pod_node[pend] == 1).all() and (s2.pod_gpu_group[pend] == 5).all()
    assert s2.node_flags[0] == 1 and s2.node_flags[2] == 0 and np.array_equal(s2.node_allocatable[:, nodes], alloc)
    others = np.setdiff1d(np.arange(snap.n_pods), pend)
    assert np.array_equal(s2.pod_status[others], snap.pod_status[others])
    # the original is untouched, and S' packs into the ABI struct (test_update_arguments_and_call_order opens it), the other arrays unchanged
    assert (snap.pod_status[pend] == 1).all()
    s2.as_struct()
    for k in snap.arrays:
        if k not in ("pod_status", "pod_node", "pod_gpu_group", "node_flags", "node_allocatable"):
            assert s2.arrays[k] is snap.arrays[k] or np.array_equal(s2.arrays[k], snap.arrays[k]), k
