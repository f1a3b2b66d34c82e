"""What kai_session_open leaves in HBM on the MI355X, against the host simulation's open.  Both fill the session context through kai_ctx_build.hpp — the library on its slab
allocator (memsets, device-to-device copies, pinned staging), the simulation on vectors — and tests/test_open_uploads.py holds the two against each other under the stand-in
runtime.  Here the same shapes are opened by the real library on the device, in a fresh child process with KAI_OPEN_DIGEST=1: every array of the context, read back before the
open's first kernel, holds the bytes the simulation's holds — but for the three arrays neither writes.  And again behind the open's kernels, which the simulation runs on
the emulator through the library's own launch sequences (kai_open_kernels.hpp): the gfx950 code and the emulated bodies leave the same bytes in every array, on these
shapes and on the small ones of tests/open_shapes.py — but for the operation log and the output staging, and the GPU-group ids where no kernel resets them."""
import os

import pytest

from test_open_uploads import ROOT, assert_sim_open_equals_library_open

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("env", [{}, {"KAI_OPEN_FULL_UPLOADS": "1"}], ids=["default", "full uploads"])
def test_the_device_holds_the_context_the_host_simulation_builds(tmp_path, env):
    lib = os.path.join(ROOT, "kai-scheduler_amd", "csrc", "libkai_core.so")
    assert os.path.exists(lib), "libkai_core.so is not built"
    assert_sim_open_equals_library_open(lib, tmp_path, env, timeout=180, behind_kernels=True)
