"""The SIMT layer's DEVICE code (the DPP scans, v_readlane / v_writelane wrappers, v_mbcnt, the inline scalar assembly, the wavefront-scope LDS atomics, v_rcp_f32 division
of kai_simt.hpp, kai_wave.hpp, kai_batch_kernels.hpp, kai_fill_buckets.hpp, kai_fill_levels.hpp) on the MI355X against the contract stated in tests/kw_conformance_cases.py:
the same bodies (tests/device_prims/kw_conformance.hpp) and the same references that tests/test_kw_conformance.py holds the emulator against.  One test per case of the table.

build() compiles tests/device_prims/libkwconf.so; without it every case FAILS.  After a launch that returned a HIP error nothing more is started on the device: every later case
of the module fails at once."""
import os

import pytest

import kw_conformance_cases as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "device_prims", "libkwconf.so")
BUILD = "hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -o tests/device_prims/libkwconf.so tests/device_prims/kw_conformance.hip   (or: python __graft_entry__.py)"
_state = {"run": None, "hip_error": None}


def _kwc_run():
    if _state["run"] is None:
        assert os.path.exists(LIB), f"{LIB} is missing; build it with: {BUILD}"
        raw = K.load_kwc_run(LIB)

        def run(body, inp, out, grid, block):
            assert _state["hip_error"] is None, _state["hip_error"]
            rc = raw(body, inp, out, grid, block)
            if rc != 0:
                _state["hip_error"] = f"an earlier launch (body {body}, grid {grid}, block {block}) returned hipError_t {rc}: nothing more is started on the device in this module"
            return rc
        _state["run"] = run
    return _state["run"]


@pytest.mark.parametrize("cid", list(K.CASES))
def test_device_against_the_contract(cid):
    assert _state["hip_error"] is None, _state["hip_error"]
    K.run_case(K.CASES[cid], _kwc_run())
