"""Spread placement on the GPU on the set-based fill kernels, on the MI355X through the C ABI: the cases of tests/test_fill_spread.py (same snapshots, same assertions) with
the spread instantiations of k_fill_levels / k_fill_counts as they run on the device — against the oracle and, where the sets ran, against the general k_fill
(KAI_FILL_GENERAL=1).  kai_action.hpp (action_stats) reports the fill kernel in bits 60 - 62 of stats.reserved[1], the rounds in reserved[4]."""
import pytest

import test_fill_spread as S
from test_gpu_parity import assert_same, gpu, on_buckets, on_counts, on_levels, run_gpu  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu


class Gpu:
    run = staticmethod(lambda snap, cfg: run_gpu(snap, cfg))
    same = staticmethod(assert_same)
    on_buckets = staticmethod(lambda res: on_buckets(res.stats))
    on_counts = staticmethod(lambda res: on_counts(res.stats))
    on_levels = staticmethod(lambda res: on_levels(res.stats))
    rounds = staticmethod(lambda res: int(res.stats.reserved[4]))


@pytest.mark.parametrize("seed", S.SEEDS)
def test_gpu_spread_random_one_divisor_clusters(gpu, seed, monkeypatch):
    S.case_random(Gpu, seed, monkeypatch)


@pytest.mark.parametrize("case", S.HAND, ids=[c.__name__[5:] for c in S.HAND])
def test_gpu_spread_hand_made(gpu, case, monkeypatch):
    case(Gpu, monkeypatch)


@pytest.mark.parametrize("case", S.HAND[:6], ids=[c.__name__[5:] for c in S.HAND[:6]])
def test_gpu_spread_hand_made_on_the_two_worker_kernel(gpu, case, monkeypatch):
    monkeypatch.setenv("KAI_FILL_TWO_WORKERS", "1")
    case(type("GpuTwo", (Gpu,), {"on_levels": staticmethod(lambda res: True)}), monkeypatch)


@pytest.mark.parametrize("case", S.DECLINES, ids=[c.__name__[13:] for c in S.DECLINES])
def test_gpu_spread_declines(gpu, case, monkeypatch):
    case(Gpu, monkeypatch)


@pytest.mark.parametrize("seed", [2, 9])
def test_gpu_spread_round_loop_on_the_device_against_the_host(gpu, seed, monkeypatch):
    S.case_round_loop(Gpu, seed, monkeypatch)


@pytest.mark.parametrize("idx,scale", S.SCALED)
def test_gpu_spread_scaled_baseline_configs(gpu, idx, scale, monkeypatch):
    S.case_scaled_config(Gpu, idx, scale, monkeypatch)
