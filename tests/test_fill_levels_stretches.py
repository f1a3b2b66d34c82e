"""kai_fill_levels.hpp, the bookkeeper's side of the command ring: a command names its job within the stretch (bits 23-28), a marker stands in front of every stretch's commands.

Random plain clusters (at most eight devices per node, so the kernel with a wavefront per level takes the fill) run through the emulator under the default, the reversed and the
randomised wavefront order (kai_simt.hpp KW_EMU_ORDER), against the oracle and — counters included — against k_fill_counts (KAI_FILL_TWO_WORKERS=1), whose counting machine books the
dead gangs itself.

The inputs must make the bookkeeper work.  Every launch over >= 1 000 planned jobs is dumped by tests/host_sim (KAI_HOSTSIM_FILL_DUMP: the planned order, the sets before the launch,
the kernel's outputs) and walked here by a model of the counting machine on the levels' populations; the model must reproduce the launch's outcomes and its number of commands, and
it tells which of the cases below a launch holds.  A seed that holds none of them, or a case no seed holds, fails the test."""
import glob
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
from test_engine_hostsim import HostSim, assert_same

abi = T.abi
synth = T.pkg.synth

BF_OK, BF_GATE, BF_DEAD = 0, 1, 2
KFL_RING, KFL_SHORT = 4096, 16
SEEDS = (0, 1, 2)
CASES = ("dead_with_commands", "dead_without_commands", "dead_first", "dead_last", "ring_wrap", "long_gang", "mixed_gang", "mismatch_mid_stretch")


def snapshot(seed):
    """(snapshot, config).  More pending pods than the cluster holds (the plan predicts the tail of every queue dead), gangs of up to 40 tasks, and every 9th gang of at least two
    tasks asks for one device on its even pods and for two on its odd ones: a gang of several classes.  Seeds 0 and 1: random clusters of a few hundred nodes; seeds 2 and 3: BASELINE
    config 5 at a tenth of its size — thousands of gangs a launch, more commands than the ring holds."""
    if seed >= 2:
        snap, cfg, _ = synth.config(4, 0.08 + 0.04 * (seed - 2), seed_offset=seed)
    else:
        snap = synth.make_snapshot((1500, 600)[seed], (14000, 30000)[seed], 7303 + seed, queue_levels=((4,), (2, 3))[seed], prefill=(0.4, 0.3)[seed], gpu_mix=((8, .7), (4, .3)),
                                   gpus_per_pod=(1, 2, 4, 8) if seed == 0 else (8,) * 31 + (1,),  # seed 1: whole nodes run out early, then stretch after stretch of dead gangs
                                   gang_sizes=(1, 2, 3, 24) if seed == 0 else (1, 2, 4, 20), gang_p=(.5, .3, .15, .05), mem_per_gpu=8 * synth.GIB, cpu_per_gpu=2000.0, zipf=True)
        cfg = abi.default_config(k_value=0.5)
    a = snap.arrays
    pending = np.nonzero(a["pod_status"][a["job_first_pod"]] == abi.POD_STATUS["Pending"])[0]
    for j in pending[::9]:
        f, n = int(a["job_first_pod"][j]), int(a["job_n_pods"][j])
        if n < 2:
            continue
        g = np.where(np.arange(n) % 2 == 0, 1.0, 2.0)
        scale = a["pod_req"][:, f] / max(a["pod_req"][abi.RES_GPU, f], 1.0)  # the gang's request per device
        for r in (abi.RES_CPU, abi.RES_MEM, abi.RES_GPU):
            a["pod_req"][r, f:f + n] = scale[r] * g if a["pod_req"][abi.RES_GPU, f] >= 1 else a["pod_req"][r, f:f + n]
    snap.finalize()
    return snap, cfg


def read_dump(prefix):
    """<prefix>.in / <prefix>.out as tests/host_sim writes them (host_sim.cpp fill_dump)"""
    with open(prefix + ".in", "rb") as f:
        raw = f.read()
    hdr = struct.unpack_from("<16i", raw, 0)
    assert hdr[0] == 0x4b464c31
    d = dict(C=hdr[1], Q=hdr[2], P=hdr[3], V=hdr[4], LV=hdr[5], NW=hdr[6])
    off = 64
    d["start"] = struct.unpack_from("<8i", raw, off)[4]; off += 32 + 80  # RoundParams, BucketParams
    d["qd"] = np.frombuffer(raw, np.float64, 64, off); off += 512
    V, P = d["V"], d["P"]
    d["flag"] = np.frombuffer(raw, np.uint8, V, off); off += V
    for k in ("first", "nt", "ucls"):
        d[k] = np.frombuffer(raw, np.int32, V, off); off += 4 * V
    d["t_cls"] = np.frombuffer(raw, np.int32, P, off); off += 4 * P
    d["words"] = np.frombuffer(raw, np.uint64, d["LV"] * d["NW"], off).reshape(d["LV"], d["NW"])
    with open(prefix + ".out", "rb") as f:
        raw = f.read()
    fs = struct.unpack_from("<6i5qQ8q", raw, 0)
    d["n_done"], d["mismatch"], d["decisions"], d["commands"] = fs[0], fs[1], fs[6], fs[18]
    d["out"] = np.frombuffer(raw, np.uint8, V, 136)
    return d


def walk(d):
    """The counting machine of kai_fill_levels.hpp on the levels' populations, stretch by stretch; returns the cases the launch holds."""
    LV, start, V = d["LV"], d["start"], d["V"]
    cnt = [0] + [int(sum(bin(int(w)).count("1") for w in d["words"][l])) for l in range(LV)]  # cnt[g]: nodes with g free devices
    qk = [int(d["qd"][k]) for k in range(d["C"])]
    found = set()
    wp = commands = decisions = 0
    n_done, mismatch = start, 0

    def level_for(q):
        for g in range(q, LV + 1):
            if cnt[g]:
                return g
        return 0

    for base in range(start, V, 64):
        if mismatch:
            break
        jn = min(64, V - base)
        cap = [0] + [sum((g // q) * cnt[g] for g in range(1, LV + 1)) for q in range(1, 65)]
        jobs = []
        for j in range(jn):
            gi = base + j
            flag, nt, ucls = int(d["flag"][gi]), int(d["nt"][gi]), int(d["ucls"][gi])
            q = 0 if ucls < 0 else min(qk[ucls], 31)
            is_def = flag == BF_DEAD and q >= 1 and cap[q] < nt
            jobs.append((flag, nt, q, is_def))
        wp += 1  # the stretch's marker
        wp0, n_out, n_cmd, defs_seen = wp, jn, 0, []
        special = set()
        for j, (flag, nt, q, is_def) in enumerate(jobs):
            gi = base + j
            if is_def:
                decisions += sum((g // q) * cnt[g] for g in range(1, LV + 1)) + 1  # the capacity at its turn, and the task that found no node
                defs_seen.append(j)
                assert d["out"][gi] == BF_DEAD
                continue
            if flag == BF_GATE:
                continue
            save, placed, cmds, fail = list(cnt), 0, 0, False
            if q == 0:
                for t in range(nt):
                    q1 = qk[int(d["t_cls"][int(d["first"][gi]) + t])]
                    g = level_for(q1) if q1 <= 31 else 0
                    if not g:
                        fail = True; break
                    cnt[g] -= 1; cnt[g - q1] += 1 if g - q1 >= 1 else 0; cmds += 1; placed += 1
            else:
                while placed < nt and not fail:
                    g = level_for(q)
                    if not g:
                        fail = True; break
                    r, rem = max(g // q, 1), nt - placed
                    k = max(min(rem // r, cnt[g]), 1); per = min(r, rem); g2 = g - per * q
                    cnt[g] -= k
                    if g2 >= 1:
                        cnt[g2] += k
                    cmds += 1; placed += k * per
            decisions += placed + (1 if fail else 0)
            if fail:
                cnt[:] = save
            else:
                n_cmd += cmds; wp += cmds
                if q == 0:
                    special.add("mixed_gang")
                elif nt > KFL_SHORT:
                    special.add("long_gang")
            assert d["out"][gi] == (BF_DEAD if fail else BF_OK), gi
            if (flag == BF_OK) == fail:
                mismatch, n_out = 1, j + 1
                break
        n_done = base + n_out
        defs = [j for j in defs_seen if j < n_out]
        commands += n_cmd
        if defs:
            found.add("dead_with_commands" if n_cmd else "dead_without_commands")
            if defs[0] == 0:
                found.add("dead_first")
            if defs[-1] == n_out - 1 and not mismatch:
                found.add("dead_last")
            if n_cmd:
                found |= special  # a long gang / a gang of several classes in a stretch whose dead gangs the bookkeeper books between its commands
        if n_cmd and wp0 // KFL_RING != (wp - 1) // KFL_RING:
            found.add("ring_wrap")  # commands of this stretch on both sides of the ring's end
        if mismatch and n_out < jn:
            found.add("mismatch_mid_stretch")
    assert (n_done, mismatch, commands, decisions) == (d["n_done"], d["mismatch"], d["commands"], d["decisions"]), "the model of the counting machine does not describe this launch"
    return found


def run_kernels(snap, cfg):
    """the fill with a wavefront per level against the oracle and against k_fill_counts, counters included"""
    stats = lambda s: (s.decisions, s.jobs_attempted, s.jobs_committed, s.rollbacks, int(s.reserved[5]))
    ref = T.Oracle.run(snap, cfg)
    res = HostSim.run(snap, cfg)
    assert int(res.stats.reserved[7]) >> 32 == 1, "the fill did not run on k_fill_levels"
    assert_same(res, ref); assert stats(res.stats)[:4] == stats(ref.stats)[:4]
    os.environ["KAI_FILL_TWO_WORKERS"] = "1"
    try:
        two = HostSim.run(snap, cfg)
    finally:
        del os.environ["KAI_FILL_TWO_WORKERS"]
    assert int(two.stats.reserved[7]) == 1, "the second run did not take k_fill_counts"
    assert_same(two, res); assert stats(two.stats) == stats(res.stats)


def test_bookkeeper_cases_against_oracle_and_counts_kernel(tmp_path, monkeypatch):
    union = set()
    for seed in SEEDS:
        pre = str(tmp_path / f"s{seed}")
        monkeypatch.setenv("KAI_HOSTSIM_FILL_DUMP", pre)
        snap, cfg = snapshot(seed)
        res = HostSim.run(snap, cfg)
        monkeypatch.delenv("KAI_HOSTSIM_FILL_DUMP")
        assert int(res.stats.reserved[7]) >> 32 == 1
        found = set()
        dumps = sorted(glob.glob(pre + "_*.in"))
        assert dumps, f"seed {seed}: no launch over 1 000 planned jobs"
        for p in dumps:
            found |= walk(read_dump(p[:-3]))
        print(f"seed {seed}: {len(dumps)} launches, cases {sorted(found)}")
        assert found, f"seed {seed} holds none of the cases: an error of this test's inputs"
        union |= found
        run_kernels(snap, cfg)
    assert union == set(CASES), f"no seed holds {sorted(set(CASES) - union)}"


@pytest.mark.parametrize("order", [1, 2])
def test_bookkeeper_cases_under_other_wave_schedules(order):
    """the same clusters with the wavefronts of the workgroup taking turns in reverse (1) and drifting apart at random (2): the setting is read once per process"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import kai_testlib as T\nimport test_fill_levels_stretches as S\n"
            "for seed in S.SEEDS:\n"
            "    S.run_kernels(*S.snapshot(seed))\n") % os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="17")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
