"""The SIMT layer (kai-scheduler_amd/csrc/kai_simt.hpp and the block-level helpers built on it) on the EMULATOR against the contract stated in tests/kw_conformance_cases.py.

The `-m "not gpu"` suite runs kernel bodies on the emulator and believes that they mean the same on gfx950.  This module pins the emulator's half of that belief, primitive by
primitive: tests/device_prims/kw_conformance.hpp (one body per group of primitives, calling the product's functions) is compiled with plain g++ and every case of the table is
held against its numpy / plain-integer reference — with the emulator's wavefronts taking turns in order, in reverse, at random and one at a time (KW_EMU_ORDER 0, 1, 2, 3; read
once per process, hence the subprocesses).  tests/test_gpu_kw_conformance.py holds the device's half against the same table."""
import glob
import json
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PRIMS = os.path.join(HERE, "device_prims")
SIM_SRC = os.path.join(PRIMS, "kw_conformance_sim.cpp")

import kw_conformance_cases as K


def sim_lib():
    so = os.path.join(PRIMS, "libkwconf_sim.so")
    deps = [SIM_SRC, os.path.join(PRIMS, "kw_conformance.hpp")] + glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.hpp")) + \
        glob.glob(os.path.join(ROOT, "kai-scheduler_amd", "csrc", "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-pthread", "-o", so, SIM_SRC])
    return so


CHILD = """
import json, sys
sys.path.insert(0, {tests!r})
import kw_conformance_cases as K
run = K.load_kwc_run({so!r})
res = {{}}
for cid, case in K.CASES.items():
    try:
        res[cid] = [K.run_case(case, run), None]
    except AssertionError as e:
        res[cid] = [0, str(e)[:800]]
print(json.dumps(res))
"""


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_every_case_on_the_emulator_against_the_contract(order):
    """all cases of the table; a case that fails is named with its first difference.  Order 3 (one wavefront at a time runs as far as it gets) is the schedule under which a
    missing barrier between two block scans on one PlanScanLds shows: under 0 .. 2 the wavefronts stay within a few collectives of each other and both calls pass without it."""
    so = sim_lib()  # built before the child starts
    env = dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="3")
    r = subprocess.run([sys.executable, "-c", CHILD.format(tests=HERE, so=so)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(res) == sorted(K.CASES), "the child ran another table"
    failed = {k: v[1] for k, v in res.items() if v[1] is not None}
    assert not failed, "\n".join(f"{k}: {v}" for k, v in failed.items())
    assert all(v[0] >= 1 for v in res.values())


def test_a_launch_with_buffers_too_small_is_refused_before_it_runs():
    """kwc_run checks the buffers against the shape before anything is launched (on the device: before anything is allocated), so that no body indexes past a buffer"""
    import numpy as np
    run = K.load_kwc_run(sim_lib())
    out = np.zeros(64, np.uint64)
    assert run(K.IDS["scan_int"], np.zeros(63, np.uint64), out, 1, 64) == 1 and run(K.IDS["scan_int"], np.zeros(64, np.uint64), out[:63], 1, 64) == 1
    assert run(K.IDS["scan_int"], np.zeros(64, np.uint64), out, 1, 2048) == 1 and run(99, np.zeros(64, np.uint64), out, 1, 64) == 1
    assert run(K.IDS["block_add3"], np.zeros(300, np.uint64), np.zeros(1200, np.uint64), 1, 100) == 1, "PlanScanLds holds whole wavefronts"
    q = np.zeros(16, np.int32); q[0] = 7  # says Q = 7 in a buffer for 3 nodes
    assert run(K.IDS["plan_setup"], q.view(np.uint64), np.zeros(64, np.uint64), 1, 128) == 1
    assert run(K.IDS["atomics"], np.zeros(3 * 64, np.uint64), np.zeros(27, np.uint64), 1, 64) == 1
    assert (out == 0).all()


def test_stand_alone_program(tmp_path):
    """-DKWC_MAIN: every body once on fixed inputs against values computed in plain C++ in that file; the waves in order and in reverse"""
    exe = str(tmp_path / "kw_conformance_sim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKWC_MAIN", "-o", exe, SIM_SRC])
    for order in ("0", "1"):
        r = subprocess.run([exe], env=dict(os.environ, KW_EMU_ORDER=order), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "kw_conformance_sim: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


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
    """the same program built with -fsanitize=address,undefined and run as its own process (nothing sanitized is loaded into Python); the options are test_stale_gangs.py's: the
    fibers switch stacks, which the stack-use-after-return mode does not follow"""
    why = _sanitizer_runtimes(tmp_path)
    if why: pytest.skip(why)
    exe = str(tmp_path / "kw_conformance_sim_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKWC_MAIN", "-o", exe, SIM_SRC])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "kw_conformance_sim: ok" in r.stdout and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-3000:]
