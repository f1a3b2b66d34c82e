"""The batch path's plan kernels on the emulator AT THE DEVICE'S WORKGROUP SIZES.

The default emulator build runs k_plan_setup and k_plan_scan with 128 threads (two wavefronts), three positions per thread and segments of 128 positions; the device runs
1 024 threads, four positions per thread and segments of 1 024 (kai_batch_kernels.hpp, kai_batch_types.hpp).  -DKAI_EMU_DEVICE_SIZES gives the emulator the device's values:
this module builds a second libhostsim with it into the test's temporary directory, selects it through KAI_HOSTSIM_SO in a child process, and holds what it computes against
the oracle and against the default-size emulator — on the snapshots of test_plan_scan_in_segments_against_one_workgroup_per_node_and_the_oracle (both settings of
KAI_PLAN_SEG_MIN), on three seeds of test_batch_under_other_wave_schedules with the wavefronts in reverse (KW_EMU_ORDER=1), and on one snapshot of the same generator with
enough single-pod jobs below one top-level queue that its stream is longer than 1 024 positions: none of the existing tests' settings reaches that (their longest stream has a
few hundred), so without it nothing here would run more than two wavefronts in k_plan_scan or cut a stream in two at the device's segment length.  The sizes a run reached are
read back from the host simulation (kai_hostsim_plan_shapes) and asserted.

Measured here: the module takes about 70 s on eight cores, the build of the second library 35 s of it."""
import json
import os
import subprocess
import sys

import pytest

import kai_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(T.ROOT, "tests", "host_sim", "host_sim.cpp")

CHILD = r"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, %(tests)r)
import numpy as np
import kai_testlib as T
from test_engine_hostsim import HostSim, assert_same
from test_batch_path import regular_snapshot, inner_limits_snapshot, stats_tuple
abi, synth = T.abi, T.pkg.synth

def long_stream_snapshot():
    # 2 600 single-pod jobs in five leaves below ONE top-level queue: with the plan's first depth of 256 jobs per leaf that queue's stream holds 1 280 positions
    return synth.make_snapshot(120, 2600, 4242, queue_levels=(1, 5), prefill=0.2, gpu_mix=((8, .6), (4, .4)), single_pod_jobs=True, gpus_per_pod=(1, 2)), abi.default_config(k_value=0.5)

def digest(res):
    h = hashlib.sha256()
    h.update(repr(res.ops).encode()); h.update(np.ascontiguousarray(res.pod_status).tobytes()); h.update(np.ascontiguousarray(res.pod_node).tobytes())
    for k in sorted(res.shares_final): h.update(np.ascontiguousarray(res.shares_final[k]).tobytes())
    return h.hexdigest()

def shapes():
    out = (C.c_int64 * 6)()
    HostSim._raw.kai_hostsim_plan_shapes(out)
    return list(out)

what = sys.argv[1]
runs = []
if what == "segments":
    both = ("1", "1000000000")  # every height below the root in segments / never
    todo = [("seg%%d" %% s,) + (inner_limits_snapshot(s) if s < 6 else (regular_snapshot(200 + s), abi.default_config(k_value=0.5))) + (both,) for s in range(10)] + [("long",) + long_stream_snapshot() + (both,)]
else:
    todo = [("reg%%d" %% s, regular_snapshot(s), abi.default_config(gpu_strategy=(abi.BINPACK, abi.SPREAD)[s %% 2], k_value=0.5), (None,)) for s in (3, 7, 29)]
    todo += [("long",) + long_stream_snapshot() + (("4096",),)]  # the device's own threshold: one workgroup per node (the emulator's default of 96 would cut the stream)
for name, snap, cfg, settings in todo:
    ref = T.Oracle.run(snap, cfg)
    for seg_min in settings:
        if seg_min is None: os.environ.pop("KAI_PLAN_SEG_MIN", None)
        else: os.environ["KAI_PLAN_SEG_MIN"] = seg_min
        HostSim.lib(); shapes()
        res = HostSim.run(snap, cfg)
        assert_same(res, ref)
        assert stats_tuple(res.stats) == stats_tuple(ref.stats), name
        assert res.stats.reserved[4] == 1, "the allocate action did not take the batch path: " + name
        runs.append(dict(name=name, seg_min=seg_min, digest=digest(res), rounds=int(res.stats.reserved[5]), stats=[int(x) for x in stats_tuple(res.stats)], shapes=shapes()))
print(json.dumps(runs))
"""


@pytest.fixture(scope="module")
def device_size_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostsim_device_sizes") / "libhostsim_device_sizes.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-DKAI_EMU_DEVICE_SIZES", "-o", so, SRC])
    return so


def default_lib():
    from test_engine_hostsim import HostSim
    HostSim.lib()  # (built before a child starts)
    return os.environ.get("KAI_HOSTSIM_SO") or os.path.join(T.ROOT, "tests", "host_sim", "libhostsim.so")


def run_child(what, so, order):
    env = dict(os.environ, KAI_HOSTSIM_SO=so, KW_EMU_ORDER=str(order), KW_EMU_SEED="5")
    env.pop("KAI_PLAN_SEG_MIN", None)
    r = subprocess.run([sys.executable, "-c", CHILD % dict(tests=HERE), what], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def compare(dev, dflt):
    assert [(r["name"], r["seg_min"]) for r in dev] == [(r["name"], r["seg_min"]) for r in dflt]
    for a, b in zip(dev, dflt):
        assert (a["digest"], a["stats"], a["rounds"]) == (b["digest"], b["stats"], b["rounds"]), f"{a['name']} (KAI_PLAN_SEG_MIN {a['seg_min']}): the device-size emulator and the default one differ"


# kai_hostsim_plan_shapes: [0] largest k_plan_scan workgroup, [1] largest k_plan_setup workgroup, [2] longest stream of a k_plan_scan node, [3] ... of a segmented node,
# [4] most segments of one node, [5] the segments' workgroup
def test_segmented_and_whole_plan_scans_at_the_device_sizes(device_size_lib):
    dev, dflt = run_child("segments", device_size_lib, 0), run_child("segments", default_lib(), 0)
    compare(dev, dflt)
    for r in dev:
        assert r["shapes"][1] == 1024, "k_plan_setup did not run its 1 024 threads"
        if r["seg_min"] == "1": assert r["shapes"][5] in (0, 256), "the segments did not run the device's workgroup"  # (0: a tree of leaves below the root has no height to cut)
    assert sum(r["shapes"][5] == 256 for r in dev) >= 6
    for r in dflt:
        assert r["shapes"][1] == 128
    seg = next(r for r in dev if r["name"] == "long" and r["seg_min"] == "1")["shapes"]
    one = next(r for r in dev if r["name"] == "long" and r["seg_min"] != "1")["shapes"]
    assert seg[3] > 1024 and seg[4] >= 2, f"no stream was cut in two at the device's segment length: {seg}"
    assert one[2] > 1024 and one[0] >= 512, f"k_plan_scan did not run more than two wavefronts on a stream of more than 1 024 positions: {one}"
    # for the record: how far the existing tests' snapshots get at these sizes (one segment, at most two wavefronts)
    print("longest streams of the segment test's snapshots:", max(r["shapes"][3] for r in dev if r["name"] != "long"), "positions; k_plan_scan workgroups up to", max(r["shapes"][0] for r in dev if r["name"] != "long"))


def test_other_wave_schedule_at_the_device_sizes(device_size_lib):
    """the wavefronts of a workgroup take their turns in reverse: sixteen of them in k_plan_setup, eight in k_plan_scan on the long stream"""
    dev, dflt = run_child("schedules", device_size_lib, 1), run_child("schedules", default_lib(), 1)
    compare(dev, dflt)
    assert all(r["shapes"][1] == 1024 for r in dev)
    lng = next(r for r in dev if r["name"] == "long")["shapes"]
    assert lng[2] > 1024 and lng[0] >= 512, lng
