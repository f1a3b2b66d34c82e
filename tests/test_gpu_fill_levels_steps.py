"""kai_fill_levels.hpp's steps held in lanes on the MI355X, through the C ABI: BASELINE config 5 at three hundredths and at a tenth of its size under bin-pack — snapshots whose
dumped launches tests/test_fill_levels_steps.py walks with its model on the CPU and certifies to hold gangs committed inside their run with three commands, one directly behind
another, and gangs that need one step more than the lanes hold — and at three hundredths under spread, whose instantiation keeps two commands a gang.  Each against the oracle and
against k_fill_counts (KAI_FILL_TWO_WORKERS=1): operations, pod states and counters equal."""
import pytest

import kai_testlib as T
import test_fill_levels_steps as M
from test_fill_levels_table import snapshot
from test_gpu_parity import assert_same, gpu, on_counts, on_levels, run_gpu, stats_tuple  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu

INPUTS = tuple(M.GPU_INPUTS)


@pytest.mark.parametrize("name", INPUTS)
def test_gpu_steps_in_lanes_against_oracle_and_counts_kernel(gpu, name, monkeypatch):
    snap, cfg = snapshot(name)
    ref = T.Oracle.run(snap, cfg)
    res = run_gpu(snap, cfg)
    assert on_levels(res.stats), "the fill did not run on k_fill_levels"
    assert_same(res, ref); assert stats_tuple(res.stats) == stats_tuple(ref.stats)
    monkeypatch.setenv("KAI_FILL_TWO_WORKERS", "1")
    two = run_gpu(snap, cfg)
    assert on_counts(two.stats) and not on_levels(two.stats)
    assert_same(two, ref); assert stats_tuple(two.stats) == stats_tuple(ref.stats)
    assert_same(res, two); assert stats_tuple(res.stats) == stats_tuple(two.stats)
