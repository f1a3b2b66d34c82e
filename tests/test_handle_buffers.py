"""The buffers that live with the handle (HandleBuf, kai-scheduler_amd/csrc/kai_handle.hpp) without a GPU: the host-only library of tests/test_open_uploads.py under
tests/handle_buffers_driver.py.  What a wrong copy of the grow-on-demand plumbing would break and no other CPU test sees: a buffer that kai_core_destroy forgets, a warm
call that allocates, a growth that leaks the old allocation or allocates twice.  (The parity of a grown handle with a fresh one on the device:
tests/test_gpu_handle_buffers.py.)"""
import json
import os
import subprocess
import sys

import pytest

from test_open_uploads import fake_lib  # noqa: F401  (fixture: the host-only library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, BYTES, PINNED = 1, 2, 8  # fakehip_image: live device allocations, their bytes, pinned bytes ever allocated


@pytest.fixture(scope="module")
def run(fake_lib):  # noqa: F811
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "handle_buffers_driver.py"), fake_lib, "all"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_every_call_succeeds_and_destroy_releases_everything(run):
    assert len(run["trace"]) == 3
    for name, rows in run["trace"].items():
        calls = [c for c, _, _ in rows]
        assert calls[:4] == ["create", "open", "update pods + nodes", "update pods"] and calls[-4:] == ["reset", "reopen", "close", "destroy"], name
        assert ("ops_apply" in calls) == ("fractions" not in name), name
        for call, rc, img in rows:
            assert rc == 0, (name, call, rc)
        assert rows[-1][2][COUNT] == 0 and rows[-1][2][BYTES] == 0, (name, "kai_core_destroy left device memory allocated", rows[-1][2])
        assert rows[-2][2][COUNT] > 0, name  # (a closed session keeps its slabs and the handle its buffers: destroy is what releases them)
    for name, g in run["growth"].items():
        assert g["rcs"] == [0] * 7, (name, g["rcs"])
        assert g["after_destroy"][COUNT] == 0 and g["after_destroy"][BYTES] == 0, name


def test_a_second_identical_call_allocates_nothing(run):
    for name, rows in run["trace"].items():
        by = {c: img for c, _, img in rows}
        pairs = [("best_nodes", "best_nodes again")] + ([("ops_apply", "ops_apply again")] if "ops_apply" in by else [])
        for a, b in pairs:
            assert by[a][COUNT] == by[b][COUNT] and by[a][BYTES] == by[b][BYTES] and by[a][PINNED] == by[b][PINNED], (name, a, by[a], by[b])
        # the second update has no node entries: smaller than the first, which sized the staging
        a, b = by["update pods + nodes"], by["update pods"]
        assert (a[COUNT], a[BYTES], a[PINNED]) == (b[COUNT], b[BYTES], b[PINNED]), (name, a, b)


@pytest.mark.parametrize("case", ["best_nodes", "ops_apply", "update", "ops_apply check-only, C2", "update, C2"])
def test_growth_frees_one_allocation_and_makes_one(run, case):
    """A warm small call, then a large one (best_nodes: 3 then 8 192 queries; ops_apply: 2 then 8 192 ALLOCATE operations on C5 at 20 %; update: 3 then 4 096 pods; the
    C2 cases: the sizes tests/test_gpu_handle_buffers.py uses).  The large call regrows the device buffer and the pinned one — the count of live allocations stays, live
    bytes and pinned bytes rise — and the same call again raises neither."""
    g = run["growth"][case]
    before, cold, warm, grown, again = g["images"]
    assert cold[COUNT] == before[COUNT] + 1 and cold[PINNED] > before[PINNED], "the first call allocates the handle's device buffer and its staging"
    assert (warm[COUNT], warm[BYTES], warm[PINNED]) == (cold[COUNT], cold[BYTES], cold[PINNED]), "a warm call allocated"
    assert grown[COUNT] == warm[COUNT], "growth: one allocation freed, one made"
    assert grown[BYTES] > warm[BYTES] and grown[PINNED] > warm[PINNED], (case, g["large"], "the large call did not regrow the buffers")
    assert (again[COUNT], again[BYTES], again[PINNED]) == (grown[COUNT], grown[BYTES], grown[PINNED]), "the same call again allocated"
