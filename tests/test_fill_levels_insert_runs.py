"""kai_fill_levels.hpp, the set workers: a RUN of insertions taken in lanes, and the lowest level's worker that hands nothing over.

A worker sees its commands in frames of up to 64.  A run of insertions is two or more commands of a frame that name the worker's level as their target with no removal at that
level between them.  Inside a run the insertions commute: they or bits into words, set summary bits and lower the level's first node.  The kernel takes the insertions of a run
that come from ONE source level in one pass — the lanes read the hand-over ring of the pair together, every entry lane ors its mask into its word, a uniform loop tells the first
summary and finds the first node, the ring moves on once —, so a run from several source levels goes by in pieces, each piece a run of its own or a single insertion; a source that
is behind sends the piece the old way, entry by entry.  The lowest level's nodes leave for no level: its worker's removals form no hand-over entry.

The model of tests/test_fill_levels_table.py (the counting machine with its decision table; bin-pack and spread) walks every input with a Levels that cuts the command stream
into frames of 64 commands — the frames of a worker that is behind; how a worker that keeps up really sees them depends on how the wavefronts take turns, which the three orders of
the emulator vary — and classifies every run it meets:
  a  two entries of a run into one word
  b2 a run from two source levels                      b3 from three
  c1 a command of several entries first in its run     c2 not first
  d  an entry below the level's first node into an empty word, with a second entry of the run in that word
  e  an entry into the cached word (the word of the first node at the run's start)
  f  a run into an empty level
  g  a removal directly behind the run takes a node the run brought
  h  a run whose entries lie on both sides of a pair ring's end, with more than KFL_XR hand-overs of that pair before it
  i  a run cut by the end of a frame
  k  a run under spread — a case of the INPUTS only: the spread instantiation of the kernel takes no runs in lanes (kai_fill_levels.hpp RUNS; DESIGN.md 5.2d has the replay that
     decided it), so for the spread snapshots the model certifies what the serial path meets, and the GPU test checks that spread still computes what it did
  l  removals of the lowest level before, between and behind runs
  s  a run whose entries lie in three summary groups
and one the model cannot see:
  j  a run reached before its source has handed over: the kernel counts the runs it took in lanes and the ones it sent the serial way (FillStatus.rescans3: low word | high word)

The inputs: two launches WRITTEN HERE in the dump's format — 256 nodes for the cases about words, rings and frames, 8 320 nodes (130 words, three summary groups) for `s` —,
replayed by tests/host_sim/fill_replay.cpp (the emulated k_fill_levels and k_fill_counts against the scalar C++ fill, every output and counter) under the three wavefront orders;
and the dumped launches of BASELINE config 5 at 0.1 and 0.03 of its size, bin-packed and spread, through HostSim — the snapshots tests/test_gpu_fill_levels_insert_runs.py runs
on the device, which relies on the cases asserted here for them.
"""
import glob
import os
import struct
import subprocess

import pytest

import kai_testlib as T
import test_fill_levels_runs as R
import test_fill_levels_table as TB
import test_fill_levels_workers as W
from test_engine_hostsim import HostSim

KFL_XR = R.KFL_XR
FRAME = 64
WRITTEN_CASES = {"a", "b2", "b3", "c1", "c2", "d", "e", "f", "g", "h", "i", "l", "s"}
# the snapshots of the GPU test and the cases each of them must hold
GPU_INPUTS = {"c5_0.1_binpack": {"a", "b2", "b3", "c1", "c2", "e", "f", "g", "i", "l"}, "c5_0.03_binpack": {"a", "b2", "b3", "c1", "c2", "e", "f", "g", "l"},
              "c5_0.1_spread": {"k", "a", "b2"}, "c5_0.03_spread": {"k", "a", "b2"}}


class RunLevels(R.Levels):
    """R.Levels, cutting the commands into frames of 64 and classifying the runs of insertions every level meets.  FOUND: the cases; RUNS: {level: runs}"""
    FOUND, RUNS, SPREAD = set(), {}, False

    def __init__(self, words):
        super().__init__(words)
        self.n_cmd = 0
        self.open = {}      # level: the run being built — dict(cmds=[(source, [(word, nodes)])], first, words0, pairs0)
        self.cut = {}       # level: commands of the run the last frame's end cut
        self.pair = {}      # (g, g2): hand-over entries so far
        self.low = 0        # the lowest level's removals and runs: R RUN R RUN R, as far as seen

    def close(self, G, removed=None):
        run = self.open.pop(G, None)
        if run is None:
            return
        cmds = run["cmds"]
        if removed is None:
            self.cut[G] = len(cmds)
        if len(cmds) < 2:
            return
        F = RunLevels.FOUND
        RunLevels.RUNS[G] = RunLevels.RUNS.get(G, 0) + 1
        if G == 1 and self.low in (1, 3):
            self.low += 1
        entries = [(s, w, ns) for s, es in cmds for w, ns in es]
        ws = [w for _, w, _ in entries]
        if len(set(ws)) < len(ws):
            F.add("a")
        srcs = {s for s, _ in cmds}
        if len(srcs) == 2:
            F.add("b2")
        if len(srcs) >= 3:
            F.add("b3")
        if len(cmds[0][1]) >= 2:
            F.add("c1")
        if any(len(es) >= 2 for _, es in cmds[1:]):
            F.add("c2")
        first = run["first"]
        if first is None:
            F.add("f")
        else:
            if any(w == first >> 6 for w in ws):
                F.add("e")
            if any(min(ns) < first and w not in run["words0"] and ws.count(w) >= 2 for _, w, ns in entries):
                F.add("d")
        if removed is not None and set(removed) & {n for _, _, ns in entries for n in ns}:
            F.add("g")
        for s in srcs:
            n0, n = run["pairs0"].get((s, G), 0), sum(1 for x, _, _ in entries if x == s)
            if n0 > KFL_XR and n0 // KFL_XR != (n0 + n - 1) // KFL_XR:
                F.add("h")
        if len({w >> 6 for w in ws}) >= 3:
            F.add("s")
        if RunLevels.SPREAD:
            F.add("k")

    def move(self, g, g2, k):
        if self.n_cmd and self.n_cmd % FRAME == 0:  # a frame's end cuts every run
            for G in list(self.open):
                self.close(G)
        self.n_cmd += 1
        nodes = sorted(self.heap[g])[:k]
        self.close(g, removed=nodes)
        self.cut.pop(g, None)
        if g == 1 and self.low in (0, 2, 4):
            self.low += 1
            if self.low == 5:
                RunLevels.FOUND.add("l")
        if g2 >= 1:
            es = []
            for n in nodes:
                if not es or es[-1][0] != n >> 6:
                    es.append((n >> 6, []))
                es[-1][1].append(n)
            if g2 not in self.open:
                if self.cut.pop(g2, 0) >= 1:
                    RunLevels.FOUND.add("i")  # the insertions on both sides of the frame's end are one run but for the cut
                tgt = self.heap[g2]
                self.open[g2] = dict(cmds=[], first=min(tgt) if tgt else None, words0={n >> 6 for n in tgt}, pairs0=dict(self.pair))
            self.open[g2]["cmds"].append((g, es))
            self.pair[(g, g2)] = self.pair.get((g, g2), 0) + len(es)
        return super().move(g, g2, k)

    def words(self, LV, NW):
        for G in list(self.open):  # the launch's end
            self.close(G)
        return super().words(LV, NW)


def walk(d, spread=False):
    """TB.walk with the classifying Levels; returns (the cases of the launch, {level: runs})"""
    RunLevels.FOUND, RunLevels.RUNS, RunLevels.SPREAD = set(), {}, spread
    keep = R.Levels
    R.Levels = RunLevels
    try:
        TB.walk(d, spread)  # (asserts that the model describes the launch: outcomes, commands, the sets it leaves)
    finally:
        R.Levels = keep
    return set(RunLevels.FOUND), dict(RunLevels.RUNS)


def run_counters(prefix):
    """(runs of insertions the emulated kernel took in lanes, runs it sent the serial way) of <prefix>.out"""
    with open(prefix + ".out", "rb") as f:
        fs = struct.unpack_from("<6i5qQ8q", f.read(136), 0)
    return fs[19] & 0xffffffff, fs[19] >> 32


QD = (7, 5, 3, 1)  # devices of class 0 .. 3: a task of 7 moves a node from level 8 to level 1, one of 5 from level 6, one of 3 from level 4; one of 1 takes a node of level 1 away
Q7, Q5, Q3, Q1 = range(4)


def launch_words(prefix):
    """256 nodes.  Levels 8, 6 and 4 are pools, levels 7, 5, 3 and 2 stay empty, so that every gang finds its nodes where the comments say; level 1 starts with 200 and 205."""
    nodes = {8: [10, 11, 63, 64, 65, 128] + list(range(129, 199)), 6: [201, 202, 203, 204], 4: [70, 71], 1: [200, 205]}
    gangs = [(Q1, 1),                # node 200 leaves level 1: a removal in front of the runs; its first node is 205, word 3
             (Q7, 1), (Q7, 1),       # nodes 10 11 -> level 1: below its first node, into word 0, which was empty — two entries of one word
             (Q5, 1),                # node 201 -> level 1 from level 6: a second source; into the cached word
             (Q1, 1),                # node 10 leaves: a removal behind the run takes a node the run brought
             (Q1, 3),                # nodes 11 201 205 leave: level 1 is empty
             (Q7, 2),                # nodes 63 64 -> the empty level: a command of two entries (words 0 and 1), first in its run
             (Q3, 1),                # node 70 -> level 1 from level 4
             (Q5, 1),                # node 202 -> level 1 from level 6: three sources
             (Q7, 2),                # nodes 65 128: a command of two entries, not first
             (Q1, 1)]                # node 63 leaves: a removal between runs
    gangs += [(Q7, 1)] * 27          # nodes 129 .. 155: entries 6 .. 32 of the pair (8, 1)
    gangs += [(Q1, 1)]
    gangs += [(Q7, 1)] * 29          # nodes 156 .. 184: entries 33 .. 61; commands 39 .. 67 of the launch: the frame's end cuts the run
    gangs += [(Q1, 1)]
    gangs += [(Q7, 1)] * 6           # nodes 185 .. 190: entries 62 .. 67, on both sides of the ring's end, 62 hand-overs before them
    gangs += [(Q1, 1)]               # a removal behind the last run
    W.write_launch(prefix, 4, nodes, QD, gangs)
    return len(gangs)


def launch_groups(prefix):
    """8 320 nodes, 130 words a level, three summary groups.  Level 1 starts with 18 nodes of word 128 (group 2); 16 removals stand in front of the run, so that level 8's
    worker has handed the run's nodes over when level 1's gets there, under every order.  The run brings two nodes of the last word of group 0, one of the first word of group 1
    and one of group 2 — three commands, four entries, the last command two of them.  The removals behind it empty word 63 and then word 64: the level's next first node is found
    through the SECOND summary, in groups 1 and 2 — the bits the run has to have set."""
    a, b, c, d = 63 * 64 + 62, 63 * 64 + 63, 64 * 64, 129 * 64 + 5
    nodes = {8: [a, b, c, d], 1: [128 * 64 + i for i in range(18)]}
    gangs = [(Q1, 1)] * 16           # removals in front of the run
    gangs += [(Q7, 1), (Q7, 1),      # nodes a b -> level 1: one word of group 0, below its first node
              (Q7, 2),               # nodes c d: two entries, groups 1 and 2
              (Q1, 2),               # nodes a b leave: word 63 and with it group 0 are empty, the first node is c — group 1, which only the run has told the second summary of
              (Q1, 1),               # c leaves: word 64 is empty, the first node is in word 128 again
              (Q1, 3)]               # the two nodes left of word 128 and d, the only node of word 129
    W.write_launch(prefix, 130, nodes, QD, gangs)
    return len(gangs)


def fill_replay(tmp):
    """tests/host_sim/fill_replay.cpp with the kernel's run counters (-DKFL_RUN_STATS), built once per directory"""
    exe = os.path.join(str(tmp), "fill_replay_stats")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-DKFL_RUN_STATS", "-o", exe, os.path.join(T.ROOT, "tests", "host_sim", "fill_replay.cpp")])
    return exe


def written(tmp, order):
    """the written launches through the kernels (all outputs and counters equal to the scalar fill's) and through the model: (cases, runs sent the serial way).  Every launch
    must have runs the kernel took IN LANES, under every order: the words launch two at the least (its runs stand behind removals of their level), the groups launch its one."""
    found, serial = set(), 0
    for name, write in (("words", launch_words), ("groups", launch_groups)):
        pre = os.path.join(str(tmp), f"{name}{order}")
        V = write(pre)
        r = subprocess.run([fill_replay(tmp), pre], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=120)  # (a written launch replays in a second or two; a worker that loses a node's trail waits for ever)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
        d = R.read_dump(pre)
        assert (d["n_done"], d["mismatch"]) == (V, 0) and all(int(x) == R.BF_OK for x in d["out"][:V]), "every gang of a written launch fits"
        f, runs = walk(d)
        print(f"{name}, order {order}: cases {sorted(f)} runs {runs} kernel (lanes, serial) {run_counters(pre)}")
        found |= f
        a, b = run_counters(pre)
        assert a >= (2 if name == "words" else 1), f"{name}, order {order}: the kernel took {a} runs of insertions in lanes ({b} went the serial way)"
        serial += b
    return found, serial


@pytest.mark.parametrize("order", [0, 1, 2])
def test_written_launches_hold_every_case(order, tmp_path):
    found, _ = written(tmp_path, order)
    assert found >= WRITTEN_CASES, f"no written launch holds {sorted(WRITTEN_CASES - found)}"


def test_a_run_reached_before_its_source_goes_the_serial_way(tmp_path):
    """case j.  Which runs a worker reaches before their source has handed over depends on how the wavefronts take turns; over the three orders some run does, and the results
    are the scalar fill's all the same (written() asserts that)"""
    serial = sum(written(tmp_path, order)[1] for order in (0, 1, 2))
    assert serial >= 1, "no run was reached before its source had handed over"


_DUMPED = {}


def dumped(name, tmp):
    """the dumped launches of a snapshot of the GPU test through HostSim (shadowed by the scalar fill) and through the model"""
    if name not in _DUMPED:
        pre = os.path.join(str(tmp), name)
        os.environ["KAI_HOSTSIM_FILL_DUMP"] = pre
        try:
            snap, cfg = TB.snapshot(name)
            res = HostSim.run(snap, cfg)
        finally:
            del os.environ["KAI_HOSTSIM_FILL_DUMP"]
        assert int(res.stats.reserved[7]) >> 32 == 1, "the fill did not run on k_fill_levels"
        dumps = sorted(glob.glob(pre + "_*.in"))
        assert dumps
        found, runs = set(), {}
        for p in dumps:
            f, r = walk(R.read_dump(p[:-3]), spread=name.endswith("spread"))
            found |= f
            for g, n in r.items():
                runs[g] = runs.get(g, 0) + n
        _DUMPED[name] = (found, runs)
    return _DUMPED[name]


@pytest.mark.parametrize("name", sorted(GPU_INPUTS))
def test_gpu_inputs_hold_their_cases(name, tmp_path):
    found, runs = dumped(name, tmp_path)
    print(f"{name}: cases {sorted(found)} runs per level {dict(sorted(runs.items()))}")
    assert GPU_INPUTS[name] <= found, f"{name} does not hold {sorted(GPU_INPUTS[name] - found)}: tests/test_gpu_fill_levels_insert_runs.py relies on it"
    # the runs the issue counted for the bin-packed snapshots, per level (its frames and these differ a little at level 1: 272 / 93 there, 296 / 100 here)
    floor = {"c5_0.1_binpack": (272, 129, 91), "c5_0.03_binpack": (93, 45, 32)}.get(name, (2, 2, 2))
    for level, n in zip((1, 2, 3), floor):
        assert runs.get(level, 0) >= n, f"{name}: level {level} meets {runs.get(level, 0)} runs of insertions, {n} expected"
