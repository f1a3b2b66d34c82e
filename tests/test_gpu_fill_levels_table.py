"""kai_fill_levels.hpp's decision table on the MI355X, through the C ABI: the snapshots whose dumped launches tests/test_fill_levels_table.py walks with its model on the CPU and
certifies to hold the cases a stale table would get wrong — the source level emptied in front of a gang of the same request (b), a target level that becomes non-empty and must be
taken by a later gang of the run (c), eight and more consecutive gangs that each change the mask (d), a mask change made by a second step (e), a level with fewer nodes than the
gang wants (i) and, under spread, the top level emptied mid-run (l): BASELINE config 5 at a tenth and at three hundredths of its size, bin-packed and spread.  Each against the
oracle, against k_fill_counts (KAI_FILL_TWO_WORKERS=1) and against the general k_fill (KAI_FILL_GENERAL=1), operations and statistics equal — the general kernel's statistics too,
which tests/test_gpu_fill_levels_workers.py, whose inputs these are, does not compare.  What is new here is on the CPU side: which cases each input holds is asserted by
tests/test_fill_levels_table.py (GPU_INPUTS)."""
import pytest

import kai_testlib as T
import test_fill_levels_table as M
from test_gpu_parity import assert_same, gpu, on_buckets, on_counts, on_levels, run_gpu, stats_tuple  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu

INPUTS = tuple(M.GPU_INPUTS)
_ORACLE = {}


def oracle(name, snap, cfg):
    if name not in _ORACLE:
        _ORACLE[name] = T.Oracle.run(snap, cfg)
    return _ORACLE[name]


@pytest.mark.parametrize("name", INPUTS)
def test_gpu_decision_table_against_oracle_counts_kernel_and_general_kernel(gpu, name, monkeypatch):
    snap, cfg = M.snapshot(name)
    ref = oracle(name, snap, cfg)
    res = run_gpu(snap, cfg)
    assert on_levels(res.stats), "the fill did not run on k_fill_levels"
    assert_same(res, ref); assert stats_tuple(res.stats) == stats_tuple(ref.stats)
    monkeypatch.setenv("KAI_FILL_TWO_WORKERS", "1")
    two = run_gpu(snap, cfg)
    assert on_counts(two.stats) and not on_levels(two.stats)
    assert_same(two, ref); assert stats_tuple(two.stats) == stats_tuple(ref.stats)
    monkeypatch.delenv("KAI_FILL_TWO_WORKERS")
    monkeypatch.setenv("KAI_FILL_GENERAL", "1")
    gen = run_gpu(snap, cfg)
    assert not on_buckets(gen.stats) and not on_levels(gen.stats) and not on_counts(gen.stats)
    assert_same(gen, ref); assert stats_tuple(gen.stats) == stats_tuple(ref.stats)
