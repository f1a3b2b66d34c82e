"""kai_fill_levels.hpp, the counting machine's runs and the set workers' usual command.

A RUN is the short gangs (one class, 1 .. KFL_SHORT tasks) in front of the next long one: the counting machine walks it without storing anything — a gang's first command is held in
lane jj of one register, a second one in another — and FLUSHES it at its end: every lane forms its own gang's commands, a prefix sum places them in the ring, head is published once.
A short gang that needs a third step ends the run in front of it and goes the long way.  The set workers take the usual command (one node, the word it sat in stays non-empty, the
hand-over ring has room) straight through, with one rarely taken exit for each of: the word is emptied, the hand-over ring has to be looked at, several nodes.

A random plain cluster (at most eight devices per node) and BASELINE config 5 at a tenth of its size run through the emulator under the default, the reversed and the randomised
wavefront order (kai_simt.hpp KW_EMU_ORDER), against the oracle and — counters included — against k_fill_counts (KAI_FILL_TWO_WORKERS=1).

The inputs must make these paths run.  Every launch over >= 1 000 planned jobs is dumped by tests/host_sim (KAI_HOSTSIM_FILL_DUMP) and its INPUTS are walked here by a model of the
counting machine (on the levels' populations) and of the levels' sets (which node a command moves, word by word); the model must reproduce the launch's outcomes, its number of
commands and the sets it leaves, and it tells which of the cases below the launch holds.  A case that no seed holds fails the test.

What the model can certify of "a full hand-over ring": a worker knows the consumer's progress as it last read it (0 at the start), so the 33rd entry of a (source, target) pair
takes the exit that reads it again — with certainty; whether the producer then also has to wait depends on how the wavefronts take turns, which the three orders vary.

One case no snapshot can hold: "first_step_failure_between_commits" (a first-step failure inside a run with committed gangs on both sides).  Gangs behind a failed one are
walked only if the failure was predicted; the plan predicts a gang of one class dead only if it asks for more tasks than cls_cap = sum over g of (g / q) x nodes of level g at the
ROUND's start (kai_fill_buckets.hpp kb_class_capacity: the formula of the counting machine's own capacities); the levels only shrink during a round, so at its stretch's start
such a gang is "dead for good" and takes no part in the walk (in the dumped launches of 23 clusters every walked gang that failed was the launch's mispredicted last job).  The
kernel's contract is wider than what the plan produces — a prediction is any of the three flags on any job — so this case is given to the kernels as a launch WRITTEN HERE in the
dump's format (synthetic_launch) and replayed by tests/host_sim/fill_replay.cpp: the emulated k_fill_levels and k_fill_counts against the scalar C++ fill, every output and counter
compared, under the three wavefront orders; the same model walks it, must describe it, and must find the case in it.
"""
import glob
import heapq
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import kai_testlib as T
import test_fill_levels_stretches as S
from test_engine_hostsim import HostSim

BF_OK, BF_GATE, BF_DEAD = S.BF_OK, S.BF_GATE, S.BF_DEAD
KFL_RING, KFL_SHORT, KFL_XR = S.KFL_RING, S.KFL_SHORT, 32
SEEDS = (0, 1)
CASES = ("run_of_64_one_step_gangs", "two_step_gang_in_run", "third_step_ends_run", "first_step_failure_between_commits", "rollback_in_run", "mismatch_mid_run",
         "flush_across_ring_end", "worker_emptied_word", "worker_handover_ring_exit", "worker_several_nodes_between_usual")


def snapshot(seed):
    """(snapshot, config).  Seed 0: a random cluster of 800 nodes with 16 000 single-pod jobs of one device — stretch after stretch of 64 one-step gangs; seed 1: BASELINE config 5
    at a tenth of its size — gangs of every size, more commands a launch than the ring holds."""
    if seed == 0:
        snap = T.pkg.synth.make_snapshot(800, 16000, 9197, queue_levels=(3,), prefill=0.2, gpu_mix=((8, .7), (4, .3)), gpus_per_pod=(1,), gang_sizes=(1,), gang_p=(1.0,),
                                         mem_per_gpu=8 * T.pkg.synth.GIB, cpu_per_gpu=2000.0, zipf=True)
        return snap, T.abi.default_config(k_value=0.5)
    snap, cfg, _ = T.pkg.synth.config(4, 0.1)
    return snap, cfg


def synthetic_launch(prefix):
    """<prefix>.in: 256 nodes, two with 8 free devices and ten with 1; classes of 1 and of 8 devices; 71 gangs of one task.  Jobs 0 - 6 ask for 8, 1, 8, 8, 1, 8, 1 devices; jobs 3
    and 5 are predicted dead, yet the two whole nodes are there at the stretch's start: they are walked, find no level at their first step — as predicted — and the one-device jobs
    behind them commit, in the same run.  Then 64 jobs of one device predicted to fit: seven do, the eighth is the misprediction that ends the launch."""
    LV, NW, C, Q = 8, 4, 2, 1
    q_cls = [1, 0, 1, 1, 0, 1, 0] + [0] * 64
    flag = [BF_OK, BF_OK, BF_OK, BF_DEAD, BF_OK, BF_DEAD, BF_OK] + [BF_OK] * 64
    V = P = len(q_cls)
    words = np.zeros((LV, NW), np.uint64); words[7, 0] = 0b11; words[0, 1] = (1 << 10) - 1
    qd = np.zeros(64, np.float64); qd[0], qd[1] = 1.0, 8.0
    with open(prefix + ".in", "wb") as f:
        f.write(struct.pack("<16i", 0x4b464c31, C, Q, P, V, LV, NW, 1, 0, NW, 0, 0, 0, 0, 0, 0))
        f.write(struct.pack("<8i", 256, 0, 0, 0, 0, 0, 0, 0))            # RoundParams: mode 0, from job 0
        f.write(struct.pack("<4i64b", LV, NW, 1, 0, *([-1] * 64)))       # BucketParams: no static class bitmaps
        f.write(qd.tobytes()); f.write(np.array(flag, np.uint8).tobytes())
        f.write(np.arange(V, dtype=np.int32).tobytes()); f.write(np.ones(V, np.int32).tobytes()); f.write(np.array(q_cls, np.int32).tobytes())
        f.write(np.array(q_cls, np.int32).tobytes()); f.write(words.tobytes())


def fill_replay(tmp):
    """tests/host_sim/fill_replay.cpp, built once per directory"""
    exe = os.path.join(str(tmp), "fill_replay")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-o", exe, os.path.join(T.ROOT, "tests", "host_sim", "fill_replay.cpp")])
    return exe


def synthetic_cases(tmp, order=0):
    """the written launch through the kernels (all outputs and counters equal to the scalar fill's) and through the model"""
    pre = os.path.join(str(tmp), f"syn{order}")
    synthetic_launch(pre)
    r = subprocess.run([fill_replay(tmp), pre], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    d = read_dump(pre)
    found, lv = walk(d)
    assert [[int(x) for x in row] for row in d["words_out"]] == lv.words(d["LV"], d["NW"]), "the model of the levels' sets does not describe the written launch"
    assert (d["n_done"], d["mismatch"]) == (15, 1) and [int(x) for x in d["out"][:7]] == [BF_OK, BF_OK, BF_OK, BF_DEAD, BF_OK, BF_DEAD, BF_OK]
    return found


RUN_LOG = None  # a list: every run's outcomes are appended to it (for choosing the inputs)


class Levels:
    """the sets of the levels as the workers keep them: level g's nodes, lowest name rank first, and how many of them each 64-node word holds"""

    def __init__(self, words):
        self.heap, self.per_word = [[]], [None]
        for row in words:
            nodes = [(w << 6) + b for w, x in enumerate(row) for b in range(64) if (int(x) >> b) & 1]
            self.heap.append(nodes)  # (ascending: a heap)
            cnt = {}
            for n in nodes:
                cnt[n >> 6] = cnt.get(n >> 6, 0) + 1
            self.per_word.append(cnt)

    def move(self, g, g2, k):
        """the first k nodes of level g move to level g2 (0: none); returns (hand-over entries = words the nodes came from, whether a word was emptied)"""
        words, emptied = [], False
        for _ in range(k):
            n = heapq.heappop(self.heap[g]); w = n >> 6
            self.per_word[g][w] -= 1
            if not self.per_word[g][w]:
                emptied = True; del self.per_word[g][w]
            if not words or words[-1] != w:
                words.append(w)
            if g2 >= 1:
                heapq.heappush(self.heap[g2], n); self.per_word[g2][w] = self.per_word[g2].get(w, 0) + 1
        return len(words), emptied

    def words(self, LV, NW):
        out = [[0] * NW for _ in range(LV)]
        for g in range(1, LV + 1):
            for n in self.heap[g]:
                out[g - 1][n >> 6] |= 1 << (n & 63)
        return out


def walk(d):
    """The counting machine of kai_fill_levels.hpp run by run, and the workers' sets command by command; returns the cases the launch holds."""
    LV, start, V = d["LV"], d["start"], d["V"]
    lv = Levels(d["words"])
    cnt = [0] + [len(lv.heap[g]) for g in range(1, LV + 1)]
    qk = [int(d["qd"][k]) for k in range(d["C"])]
    found = set()
    wp = commands = 0
    n_done, mismatch = start, 0
    pair_entries = {}           # (g, g2): hand-over entries written so far
    last_src = {}               # g: the last two source commands of level g, "usual" (one node) or "several"

    def level_for(q):
        for g in range(q, LV + 1):
            if cnt[g]:
                return g
        return 0

    def step(q, rem):
        g = level_for(q)
        if not g:
            return None
        r = max(g // q, 1)
        k = max(min(rem // r, cnt[g]), 1); per = min(r, rem); g2 = g - per * q
        cnt[g] -= k
        if g2 >= 1:
            cnt[g2] += k
        return (g, max(g2, 0), k, per)

    def execute(cmds):
        """the workers' side of published commands"""
        nonlocal commands
        for g, g2, k, _ in cmds:
            commands += 1
            entries, emptied = lv.move(g, g2, k)
            kind = "usual" if k == 1 else "several"
            if k == 1 and emptied:
                found.add("worker_emptied_word")
            if g2 >= 1:
                before = pair_entries.get((g, g2), 0); pair_entries[(g, g2)] = before + entries
                if k == 1 and before >= KFL_XR and before % KFL_XR == 0:
                    found.add("worker_handover_ring_exit")  # (at the latest here the producer's view of the consumer's progress, read KFL_XR entries ago, says "full")
            hist = last_src.setdefault(g, [])
            hist.append(kind)
            if hist[-3:] == ["usual", "several", "usual"]:
                found.add("worker_several_nodes_between_usual")

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
            jobs.append((flag, nt, q, is_def, q == 0 or nt > KFL_SHORT or nt < 1))
        wp += 1  # the stretch's marker
        n_out = jn
        todo = [j for j, (flag, nt, q, is_def, _) in enumerate(jobs) if flag != BF_GATE and not is_def]
        run = []  # the run being walked: (outcome, commands) per gang — "ok1" / "ok2" / "fail1" (first step) / "fail2" (a later step, rolled back)

        def flush():
            nonlocal wp
            cmds = [c for o, cs in run if o in ("ok1", "ok2") for c in cs]
            outs = [o for o, _ in run]
            if RUN_LOG is not None:
                RUN_LOG.append(outs)
            if len(run) == 64 and all(o == "ok1" for o in outs):
                found.add("run_of_64_one_step_gangs")
            if "ok2" in outs:
                found.add("two_step_gang_in_run")
            if "fail2" in outs:
                found.add("rollback_in_run")
            for i, o in enumerate(outs):
                if o == "fail1" and any(x.startswith("ok") for x in outs[:i]) and any(x.startswith("ok") for x in outs[i + 1:]):
                    found.add("first_step_failure_between_commits")
            if len(cmds) >= 2 and wp // KFL_RING != (wp + len(cmds) - 1) // KFL_RING:
                found.add("flush_across_ring_end")
            wp += len(cmds)
            execute(cmds)
            run.clear()

        for ti, j in enumerate(todo):
            flag, nt, q, _, long_way = jobs[j]
            gi = base + j
            save, placed, cmds, fail = list(cnt), 0, [], False
            in_run = not long_way
            if q == 0:
                for t in range(nt):
                    q1 = qk[int(d["t_cls"][int(d["first"][gi]) + t])]
                    g = level_for(q1) if q1 <= 31 else 0
                    if not g:
                        fail = True; break
                    cnt[g] -= 1
                    if g - q1 >= 1:
                        cnt[g - q1] += 1
                    cmds.append((g, max(g - q1, 0), 1, 1)); placed += 1
            else:
                while placed < nt and not fail:
                    c = step(q, nt - placed)
                    if c is None:
                        fail = True; break
                    cmds.append(c); placed += c[2] * c[3]
                    if in_run and len(cmds) == 3:
                        found.add("third_step_ends_run"); in_run = False  # the run ends in front of this gang, which goes the long way from the start (to the same end)
            if fail:
                cnt[:] = save
            if not in_run:
                if run:
                    flush()
                if not fail:
                    wp += len(cmds); execute(cmds)
            else:
                run.append((("fail1" if not cmds else "fail2") if fail else ("ok1" if len(cmds) == 1 else "ok2"), cmds))
            assert d["out"][gi] == (BF_DEAD if fail else BF_OK), gi
            if (flag == BF_OK) == fail:
                mismatch, n_out = 1, j + 1
                if in_run and ti + 1 < len(todo) and not jobs[todo[ti + 1]][4]:
                    found.add("mismatch_mid_run")  # short gangs of the same run stand behind the job that ends the round
                break
        if run:
            flush()
        n_done = base + n_out
        for j in range(n_out):
            if jobs[j][3]:
                assert d["out"][base + j] == BF_DEAD  # dead for good
    assert (n_done, mismatch, commands) == (d["n_done"], d["mismatch"], d["commands"]), "the model of the counting machine does not describe this launch"
    return found, lv


def read_dump(prefix):
    d = S.read_dump(prefix)
    with open(prefix + ".out", "rb") as f:
        raw = f.read()
    import numpy as np
    V, P = d["V"], d["P"]
    off = 136 + V + 4 * V + 4 * V + 4 * P  # FillStatus, g_out, g_opoff, g_stmt, t_node
    d["words_out"] = np.frombuffer(raw, np.uint64, d["LV"] * d["NW"], off).reshape(d["LV"], d["NW"])
    return d


def cases_of(seed, tmp):
    pre = os.path.join(str(tmp), f"r{seed}")
    os.environ["KAI_HOSTSIM_FILL_DUMP"] = pre
    try:
        snap, cfg = snapshot(seed)
        res = HostSim.run(snap, cfg)
    finally:
        del os.environ["KAI_HOSTSIM_FILL_DUMP"]
    assert int(res.stats.reserved[7]) >> 32 == 1, "the fill did not run on k_fill_levels"
    dumps = sorted(glob.glob(pre + "_*.in"))
    assert dumps, f"seed {seed}: no launch over 1 000 planned jobs"
    found = set()
    for p in dumps:
        d = read_dump(p[:-3])
        f, lv = walk(d)
        assert [[int(x) for x in row] for row in d["words_out"]] == lv.words(d["LV"], d["NW"]), "the model of the levels' sets does not describe this launch"
        found |= f
    return found, snap, cfg


def test_inputs_hold_every_case(tmp_path):
    """the model describes every dumped launch (outcomes, commands, the sets it leaves) and finds every case in the inputs — nine in the dumped launches of the snapshots, the tenth in the written launch (module docstring)"""
    union = set()
    for seed in SEEDS:
        found, _, _ = cases_of(seed, tmp_path)
        print(f"seed {seed}: cases {sorted(found)}")
        assert found, f"seed {seed} holds none of the cases: an error of this test's inputs"
        union |= found
    assert "first_step_failure_between_commits" not in union, "a snapshot holds the case after all: the written launch is no longer needed for it"
    syn = synthetic_cases(tmp_path)
    print(f"written launch: cases {sorted(syn)}")
    assert "first_step_failure_between_commits" in syn
    union |= syn
    assert union == set(CASES), f"no input holds {sorted(set(CASES) - union)}"


def test_runs_and_workers_against_oracle_and_counts_kernel():
    for seed in SEEDS:
        S.run_kernels(*snapshot(seed))


@pytest.mark.parametrize("order", [1, 2])
def test_runs_and_workers_under_other_wave_schedules(order):
    """the same clusters with the wavefronts of the workgroup taking turns in reverse (1) and drifting apart at random (2): the setting is read once per process"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import kai_testlib as T\nimport test_fill_levels_stretches as S\nimport test_fill_levels_runs as R\n"
            "for seed in R.SEEDS:\n"
            "    S.run_kernels(*R.snapshot(seed))\n") % os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("order", [1, 2])
def test_written_launch_under_other_wave_schedules(order, tmp_path):
    assert "first_step_failure_between_commits" in synthetic_cases(tmp_path, order)
