"""The session-open, action-init and drain kernels (kai_open_kernels.hpp) on the emulator, at the smallest shapes at which they can go wrong (tests/open_shapes.py) and
under every wavefront schedule of kai_simt.hpp (KW_EMU_ORDER 0 .. 3, read once per process: a child each; 3 runs one wavefront at a time as far as it gets, the
schedule that shows a missing barrier between two heights of k_tree_usage).  The host simulation launches them through the library's own sequences with the library's
grids and blocks, so a lane stride, a partial last workgroup or a fold that leans on the wavefronts' order shows here: the open state and one allocate cycle are the
oracle's, and every array of the context behind the open's kernels holds the same bytes whatever the schedule."""
import functools
import json
import os
import subprocess
import sys

import pytest

CHILD = r'''
import ctypes as C, hashlib, json, sys
sys.path.insert(0, TESTS)
import kai_testlib as T
from test_engine_hostsim import HostSim, assert_same
import open_shapes
out = {}
for name, snap, cfg, shared in open_shapes.shapes():
    ref = T.Oracle.run(snap, cfg); res = HostSim.run(snap, cfg)
    assert_same(res, ref)
    st = snap.as_struct(); n = C.c_int64(0)
    assert HostSim._raw.kai_hostsim_open_digest(C.byref(cfg), C.byref(st), None, C.c_int64(0), C.byref(n)) == 0, name
    buf = C.create_string_buffer(n.value + 1)
    assert HostSim._raw.kai_hostsim_open_digest(C.byref(cfg), C.byref(st), buf, C.c_int64(n.value), C.byref(n)) == 0, name
    assert buf.raw[:n.value].count(b"kai open digest behind the kernels: field") > 100, name
    out[name] = [T.ops_sha256(res.ops), T.state_sha256(res), hashlib.sha256(buf.raw[:n.value]).hexdigest(), int(res.stats.reserved[2])]
print(json.dumps(out))
'''


@functools.lru_cache(maxsize=None)
def cycle_under(order):
    """every shape's (operations, final state, open digests, drained jobs) with the emulator's wavefronts scheduled by `order`; asserts inside that each is the oracle's"""
    from test_engine_hostsim import HostSim
    HostSim.lib()  # (builds tests/host_sim/libhostsim.so when it is stale, before the children look)
    env = dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="13")
    # (one wavefront at a time is no schedule for the batch path's fill kernels, whose wavefronts poll each other — kai_simt.hpp; there the allocate action runs on the
    # sequential engine, between the same action-init and drain kernels, and ends with the same operations and state)
    if order == 3: env["KAI_HOSTSIM_NO_BATCH"] = "1"
    r = subprocess.run([sys.executable, "-c", f"TESTS = {os.path.dirname(os.path.abspath(__file__))!r}\n" + CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_open_and_one_allocate_cycle_are_the_oracles(order):
    got = cycle_under(order)
    assert len(got) == 8
    assert any(v[3] > 0 for v in got.values())  # (the drain kernel had jobs to turn away)


def test_every_wave_schedule_leaves_the_same_bytes():
    first = {k: v[:3] for k, v in cycle_under(0).items()}  # (operations, final state, the context behind the open's kernels)
    for order in (1, 2, 3):
        assert {k: v[:3] for k, v in cycle_under(order).items()} == first, order
