"""kai_fill_levels.hpp's set workers on the MI355X, through the C ABI — runs of insertions taken in lanes, the lowest level's worker that hands nothing over: the snapshots whose
launches tests/test_fill_levels_insert_runs.py walks with its model on the CPU — BASELINE config 5 at a tenth and at three hundredths of its size, bin-packed and spread — and the
800-node cluster of single-pod jobs, against the oracle, against k_fill_counts (KAI_FILL_TWO_WORKERS=1) and against the general k_fill (KAI_FILL_GENERAL=1).  Runs from one, two
and three source levels, runs holding commands of several entries, runs into empty levels and into the cached word, runs cut by a frame's end and removals of the lowest level
around runs are what the CPU test certifies for the bin-packed inputs; the spread instantiation takes no runs in lanes, its snapshots check that spread computes what it did.
(That the device takes runs in lanes shows in the -DKFL_PROF replay of profiles/r14_fill_levels_insert_runs.txt: the product kernel carries no counter for it.)"""
import pytest

import kai_testlib as T
import test_fill_levels_runs as R
from test_gpu_parity import assert_same, gpu, on_buckets, on_counts, on_levels, run_gpu, stats_tuple  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu

INPUTS = ("c5_0.1_binpack", "c5_0.1_spread", "c5_0.03_binpack", "c5_0.03_spread", "single_pods_800")
_ORACLE = {}


def snapshot(name):
    if name == "single_pods_800":
        return R.snapshot(0)
    _, scale, strategy = name.split("_")
    snap, cfg, _ = T.pkg.synth.config(4, float(scale))
    if strategy == "spread":
        cfg.gpu_strategy = T.abi.SPREAD
    return snap, cfg


def oracle(name, snap, cfg):
    if name not in _ORACLE:
        _ORACLE[name] = T.Oracle.run(snap, cfg)
    return _ORACLE[name]


@pytest.mark.parametrize("name", INPUTS)
def test_gpu_insert_runs_against_oracle_counts_kernel_and_general_kernel(gpu, name, monkeypatch):
    snap, cfg = snapshot(name)
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
    assert not on_buckets(gen.stats)
    assert_same(gen, ref)
