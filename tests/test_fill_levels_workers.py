"""kai_fill_levels.hpp, the set workers: a command of several nodes word by word without a loop over its nodes, the level's first summary in the worker's lanes, insertions that
read nothing.

A worker takes the first m = min(k, nodes of the cached word) nodes out of the word that holds its level's first node with one ballot (lane i ranks bit i of the word), writes the
tasks' nodes from the lanes that hold them and hands (word, mask) over in ONE entry; a command whose nodes span words goes on to the next word.  The first summary of its level
lives in its lanes (lane j: the words of group j that hold a node), so "the word is empty now" and "the word was empty" are lane writes, and an insertion merges its bits into the
word without reading it: only an insertion below the level's first node changes the cached word, and then the word it goes into was empty or is the cached one.

The model of tests/test_fill_levels_runs.py (the counting machine run by run, the levels' sets command by command) walks every input here with a Levels that classifies each
removal and each hand-over entry into the cases below.  The inputs:
  * two launches WRITTEN HERE in the dump's format, the smallest that hold the cases: 256 nodes (four words a level) for the cases about words, 8 320 nodes (130 words, three
    summary groups, a handful of nodes) for the cases about groups; a few one-class gangs of 1 .. 4 tasks each.  tests/host_sim/fill_replay.cpp replays them — the emulated
    k_fill_levels and k_fill_counts against the scalar C++ fill, every output and counter — under the three wavefront orders (KW_EMU_ORDER 0 / 1 / 2);
  * BASELINE config 5 at a tenth of its size through HostSim (its launches shadowed by the scalar fill, its result checked against the oracle by the other tests of this directory),
    the dumped launches walked by the model: 103 words a level, and removals of several nodes, emptied words, emptied levels and insertions into the empty level at levels 1 - 3.
The model must reproduce outcomes, command count and the sets left; every case must be found in some input.

One case of the list cannot exist, and the test asserts that no input holds it: "insert_other_word_below", an insertion into a non-empty word other than the cached one BELOW the
level's first node.  A non-empty word w that is not the cached word cw holds nodes at or above the first node, which sits in cw, so w > cw and every node of w lies above the
first node.  (The kernel relies on it: an insertion that lowers the first node sets the cached word to the entry's mask or merges into it, and reads nothing.)
"""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import kai_testlib as T
import test_fill_levels_runs as R
from test_engine_hostsim import HostSim

BF_OK = R.BF_OK
CASES = ("several_in_cached_word_stays", "several_empty_word_exactly", "several_over_two_words", "several_over_two_groups", "several_empty_level", "one_node_empties_level",
         "insert_empty_level", "insert_empty_word_below", "insert_empty_word_above", "insert_other_word_above", "insert_cached_word", "insert_two_entries", "refill_crosses_group")
IMPOSSIBLE = "insert_other_word_below"


class WorkerLevels(R.Levels):
    """R.Levels, telling for every command what the source level's worker and the target level's worker meet; EVENTS collects (case, level)"""
    EVENTS = set()

    def note(self, case, level):
        WorkerLevels.EVENTS.add((case, level))

    def move(self, g, g2, k):
        src, cnt = self.heap[g], self.per_word[g]
        nodes = sorted(src)[:k]  # (a heap's list is no sorted list)
        words = sorted({n >> 6 for n in nodes})
        cw = nodes[0] >> 6
        assert cw == min(cnt), "the level's first node sits in its lowest non-empty word"
        took = {w: sum(1 for n in nodes if n >> 6 == w) for w in words}
        if k > 1:
            if len(words) == 1 and took[cw] < cnt[cw]:
                self.note("several_in_cached_word_stays", g)
            if len(words) == 1 and took[cw] == cnt[cw]:
                self.note("several_empty_word_exactly", g)
            if len(words) >= 2:
                self.note("several_over_two_words", g)
            if len({w >> 6 for w in words}) >= 2:
                self.note("several_over_two_groups", g)
            if k == len(src):
                self.note("several_empty_level", g)
            if g2 >= 1 and len(words) == 2:
                self.note("insert_two_entries", g2)
        elif len(src) == 1:
            self.note("one_node_empties_level", g)
        for w in words:  # a word the command empties: where the level's next first node is found
            if took[w] == cnt[w]:
                self.note("word_emptied", g)
                rest = [x for x in cnt if x > w]
                if rest and min(rest) >> 6 != w >> 6:
                    self.note("refill_crosses_group", g)
        if g2 >= 1:  # the target's side, entry by entry (an entry: the command's nodes of one word), as the level is when the entry arrives
            tgt = {n >> 6 for n in self.heap[g2]}
            first = min(self.heap[g2]) if self.heap[g2] else None
            for w in words:
                n = min(x for x in nodes if x >> 6 == w)
                if first is None:
                    self.note("insert_empty_level", g2)
                elif w == first >> 6:
                    self.note("insert_cached_word", g2)
                elif w not in tgt:
                    self.note("insert_empty_word_below" if n < first else "insert_empty_word_above", g2)
                else:
                    self.note("insert_other_word_below" if n < first else "insert_other_word_above", g2)
                tgt.add(w); first = n if first is None else min(first, n)
        return super().move(g, g2, k)


def walk(d):
    """R.walk with the classifying Levels; returns the (case, level) pairs of the launch"""
    WorkerLevels.EVENTS = set()
    keep = R.Levels
    R.Levels = WorkerLevels
    try:
        _, lv = R.walk(d)
    finally:
        R.Levels = keep
    assert [[int(x) for x in row] for row in d["words_out"]] == lv.words(d["LV"], d["NW"]), "the model of the levels' sets does not describe this launch"
    return set(WorkerLevels.EVENTS)


def write_launch(prefix, NW, nodes, qd, gangs):
    """<prefix>.in in the dump's format.  nodes: {level: [node, ..]}; qd: the classes' devices; gangs: [(class, tasks)], every one predicted to fit"""
    LV, C, Q = 8, len(qd), 1
    V = len(gangs); nt = [n for _, n in gangs]; P = sum(nt)
    first = np.concatenate(([0], np.cumsum(nt)[:-1])).astype(np.int32)
    ucls = np.array([c for c, _ in gangs], np.int32)
    t_cls = np.repeat(ucls, nt).astype(np.int32)
    words = np.zeros((LV, NW), np.uint64)
    for g, ns in nodes.items():
        for n in ns:
            words[g - 1, n >> 6] |= np.uint64(1 << (n & 63))
    q = np.zeros(64, np.float64); q[:C] = qd
    nw1 = (NW + 63) // 64
    with open(prefix + ".in", "wb") as f:
        f.write(struct.pack("<16i", 0x4b464c31, C, Q, P, V, LV, NW, nw1, 0, NW, 0, 0, 0, 0, 0, 0))
        f.write(struct.pack("<8i", 256, 0, 0, 0, 0, 0, 0, 0))            # RoundParams: mode 0, from job 0
        f.write(struct.pack("<4i64b", LV, NW, nw1, 0, *([-1] * 64)))     # BucketParams: no static class bitmaps
        f.write(q.tobytes()); f.write(np.full(V, BF_OK, np.uint8).tobytes())
        f.write(first.tobytes()); f.write(np.array(nt, np.int32).tobytes()); f.write(ucls.tobytes()); f.write(t_cls.tobytes()); f.write(words.tobytes())


QD = (8, 5, 6, 4, 3, 2)  # devices of class 0 .. 5
Q8, Q5, Q6, Q4, Q3, Q2 = range(6)


def launch_words(prefix):
    """256 nodes.  Level 8 is the pool; a gang of 8 devices takes whole nodes away, one of 5 moves nodes to level 3, one of 6 to level 2, one of 4 puts two tasks on a node;
    gangs of 3 and of 2 devices then take level 3's and level 2's nodes.  Level 3 starts with node 202 alone, so that the first node that arrives lies below it."""
    nodes = {8: list(range(12)) + [67, 68, 133, 134, 212, 213, 214, 222, 223], 3: [202]}
    gangs = [(Q8, 3),   # nodes 0 1 2 of the cached word, which stays
             (Q5, 1),   # node 3 -> level 3: into an empty word, below its first node (202)
             (Q5, 1),   # node 4 -> level 3: into the cached word
             (Q4, 4),   # nodes 5 6, two tasks on each
             (Q6, 1),   # node 7 -> level 2: into an empty level
             (Q2, 1),   # node 7 leaves level 2: one node, the level is emptied
             (Q8, 4),   # nodes 8 .. 11: the word is emptied exactly
             (Q5, 1),   # node 67 -> level 3: an empty word above the first node
             (Q5, 2),   # nodes 68 133: two words, two entries; level 3 takes 68 into a non-empty word that is not the cached one
             (Q5, 1),   # node 134 -> level 3, beside 133
             (Q5, 1),   # node 212 -> level 3, beside 202
             (Q8, 4),   # nodes 213 214 222 223: the level is emptied
             (Q3, 2),   # level 3: nodes 3 4, its first word emptied exactly
             (Q3, 3),   # level 3: nodes 67 68 133, two words
             (Q3, 1)]   # level 3: node 134, the word emptied by one node
    write_launch(prefix, 4, nodes, QD, gangs)
    return len(gangs)


def launch_groups(prefix):
    """8 320 nodes, 130 words a level, three summary groups: level 8 holds two nodes in the last word of group 0, one in the first word of group 1 and two in group 2"""
    a, b, c = 63 * 64 + 62, 63 * 64 + 63, 64 * 64
    nodes = {8: [a, b, c, 129 * 64 + 5, 129 * 64 + 6]}
    gangs = [(Q8, 1),   # node a
             (Q5, 2),   # nodes b c -> level 3: two words of two groups; level 8 goes on in group 2
             (Q3, 1),   # level 3: node b leaves, its first node is now in the next group
             (Q8, 2)]   # the last two nodes of level 8
    write_launch(prefix, 130, nodes, QD, gangs)
    return len(gangs)


def written_cases(tmp, order=0):
    """the written launches through the kernels (all outputs and counters equal to the scalar fill's) and through the model"""
    found = set()
    for name, write in (("words", launch_words), ("groups", launch_groups)):
        pre = os.path.join(str(tmp), f"{name}{order}")
        V = write(pre)
        r = subprocess.run([R.fill_replay(tmp), pre], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
        d = R.read_dump(pre)
        assert (d["n_done"], d["mismatch"]) == (V, 0) and all(int(x) == BF_OK for x in d["out"][:V]), "every gang of a written launch fits"
        found |= walk(d)
    return found


def names(found):
    return {c for c, _ in found}


@pytest.mark.parametrize("order", [0, 1, 2])
def test_written_launches_hold_every_case(order, tmp_path):
    found = written_cases(tmp_path, order)
    print(f"written launches, order {order}: {sorted(found)}")
    assert IMPOSSIBLE not in names(found)
    assert names(found) - {"word_emptied"} == set(CASES), f"no written launch holds {sorted(set(CASES) - names(found))}"


def test_config5_at_a_tenth_holds_the_hot_levels_cases(tmp_path):
    """config 5 at a tenth of its size: the model describes every dumped launch, and levels 1 - 3 see removals of several nodes, emptied words and emptied levels"""
    pre = os.path.join(str(tmp_path), "c5")
    os.environ["KAI_HOSTSIM_FILL_DUMP"] = pre
    try:
        snap, cfg = R.snapshot(1)
        res = HostSim.run(snap, cfg)
    finally:
        del os.environ["KAI_HOSTSIM_FILL_DUMP"]
    assert int(res.stats.reserved[7]) >> 32 == 1, "the fill did not run on k_fill_levels"
    dumps = sorted(glob.glob(pre + "_*.in"))
    assert dumps
    found = set()
    for p in dumps:
        d = R.read_dump(p[:-3])
        assert d["NW"] == 103
        found |= walk(d)
    print(f"config 5 at 0.1: {sorted(found)}")
    assert IMPOSSIBLE not in names(found)
    for level in (1, 2, 3):
        several = {c for c, l in found if l == level and c.startswith("several_")}
        assert several, f"level {level}: no removal of several nodes"
        assert ("word_emptied", level) in found, f"level {level}: no emptied word"
        assert {("several_empty_level", level), ("one_node_empties_level", level)} & found, f"level {level}: never emptied"
        assert ("insert_empty_level", level) in found, f"level {level}: no insertion into the empty level"
