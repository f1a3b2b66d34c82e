"""kai_fill_levels.hpp, the counting machine's decision table.

Per stretch, lane j holds job j's FIRST step under one mask of non-empty levels as one word (level, target level, tasks per node, the nodes the gang wants, "that is all of it",
"a level was found", "not what the plan predicted"); a run's usual gang reads its word, takes k = min(kq, nodes of the level) and updates two counts and the mask.  The table is
exact for the mask it was built for and is rebuilt before the next gang reads its word whenever the mask differs — after a first step, a second step, a rollback, a third step
that ends the run, a long gang, a new stretch.  A stale word is a plausible wrong answer (a level that is no longer the lowest, or one that is empty), so the inputs must make every
way the mask can change under a run happen.

A model of the counting machine walks the INPUTS of dumped launches (tests/host_sim, KAI_HOSTSIM_FILL_DUMP) and of launches written here in the dump's format: gang by gang it
reads the word of a table kept the way the kernel keeps it, checks it against the step computed from the live counts, reproduces the launch's outcomes, its number of commands
and the sets it leaves, and tells which of the cases below the launch holds.  A case that no input holds fails the test.

The written launches (256 nodes, at most 200 jobs) are replayed by tests/host_sim/fill_replay.cpp — the emulated k_fill_levels and k_fill_counts against the scalar C++ fill,
every output and counter compared — under the three wavefront orders (kai_simt.hpp KW_EMU_ORDER), and so are the bin-packed dumped launches of the smallest snapshot; the
snapshots themselves run through the emulator against the oracle and against k_fill_counts in tests/test_fill_levels_runs.py / test_fill_levels_workers.py and, for spread, here.
fill_replay.cpp replays bin-pack only, so case (l) comes from the spread snapshots.

Cases:
  a  a run of 64 gangs with no mask change
  b  the source level is emptied, and the next gang of the same q takes the next level
  c  the target level becomes non-empty, and a later gang of the same run with q <= g2 takes the new, lower level (the stale word would name a higher one)
  d  at least 8 consecutive gangs of a run that each change the mask
  e  a mask change made by a second step
  f  a second-step rollback that restores a mask the first step had changed
  g  a third step that ends a run behind mask changes
  h  a misprediction directly behind a mask change (nothing behind it is walked or published: the launch ends there)
  i  a level holding fewer nodes than the gang wants
  j  a walked gang whose word says "no level" inside a run with commits on both sides (written launch only, see test_fill_levels_runs.py)
  k  a mask change in a stretch's last gang, followed by the first gang of the next stretch
  l  under spread, the top level emptied mid-run
"""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import kai_testlib as T
import test_fill_levels_runs as R
import test_fill_levels_stretches as S
from test_engine_hostsim import HostSim, assert_same

BF_OK, BF_GATE, BF_DEAD = S.BF_OK, S.BF_GATE, S.BF_DEAD
KFL_SHORT = S.KFL_SHORT
CASES = tuple("abcdefghijkl")
# the snapshots of tests/test_gpu_fill_levels_table.py and the cases each of them must hold (asserted below: the GPU test relies on it)
GPU_INPUTS = {"c5_0.1_binpack": set("bcdei"), "c5_0.03_binpack": set("bcdei"), "c5_0.1_spread": set("l"), "c5_0.03_spread": set("l")}


def snapshot(name):
    if name == "single_pods_800":
        return R.snapshot(0)
    _, scale, strategy = name.split("_")
    snap, cfg, _ = T.pkg.synth.config(4, float(scale))
    if strategy == "spread":
        cfg.gpu_strategy = T.abi.SPREAD
    return snap, cfg


def level_for(q, mask, spread):
    """the level a gang of q devices per task takes under the mask of non-empty levels (bit g: level g), 0 = none"""
    if not (mask >> q):
        return 0
    if spread:
        return mask.bit_length() - 1
    g = q
    while not (mask >> g) & 1:
        g += 1
    return g


def table_word(q, nt, mask, spread):
    """a job's first step as the table holds it: (g, g2, per, kq, whole) — a pure function of the job and the mask; None: no level"""
    g = level_for(q, mask, spread)
    if not g:
        return None
    r = 1 if spread else max(g // q, 1)
    kq = max(nt if spread else nt // r, 1)
    per = min(r, nt)
    return g, g - per * q, per, kq, kq * per >= nt


def walk(d, spread=False):
    """The counting machine of kai_fill_levels.hpp with its decision table, run by run; returns (cases the launch holds, the sets it leaves, counts for the write-up)."""
    LV, start, V = d["LV"], d["start"], d["V"]
    lv = R.Levels(d["words"])
    cnt = [0] + [len(lv.heap[g]) for g in range(1, LV + 1)]
    qk = [int(d["qd"][k]) for k in range(d["C"])]
    found = set()
    stats = dict(walked=0, flips=0, steps=0, clamped=0, second=0, rebuilds=0, runs=0)
    commands = 0
    n_done, mismatch = start, 0
    prev_last = None  # the last walked gang of the previous stretch: (in a run, changed the mask)

    def mask():
        return 1 | sum(1 << g for g in range(1, LV + 1) if cnt[g])

    def live_step(q, rem):
        """one step from the live counts (the kernel's general step): (g, g2, k, per, kq) or None"""
        g = level_for(q, mask(), spread)
        if not g:
            return None
        r = 1 if spread else max(g // q, 1)
        kq = max(rem if spread else rem // r, 1)
        per = min(r, rem)
        return g, max(g - per * q, 0), min(kq, cnt[g]), per, kq

    def apply(g, g2, k):
        cnt[g] -= k
        if g2 >= 1:
            cnt[g2] += k

    def publish(cmds):
        nonlocal commands
        for g, g2, k, _ in cmds:
            commands += 1
            lv.move(g, g2, k)

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
        n_out = jn
        todo = [j for j, (flag, nt, q, is_def, _) in enumerate(jobs) if flag != BF_GATE and not is_def]
        tab_mask = None  # (a new stretch: no table yet)
        run = []  # the run being walked, per gang: dict(out, cmds, q, before, after, first_after, g2new)
        last = None

        def flush():
            outs = [x["out"] for x in run]
            stats["runs"] += 1
            if len(run) == 64 and all(o == "ok1" for o in outs) and all(x["before"] == x["after"] for x in run):
                found.add("a")
            streak = 0
            for i, x in enumerate(run):
                streak = streak + 1 if x["after"] != x["before"] else 0
                if streak >= 8:
                    found.add("d")
                if x["out"] == "fail1" and any(o.startswith("ok") for o in outs[:i]) and any(o.startswith("ok") for o in outs[i + 1:]):
                    found.add("j")
                if spread and x["emptied_top"] and i + 1 < len(run):
                    found.add("l")
            publish([c for x in run if x["out"] in ("ok1", "ok2") for c in x["cmds"]])
            run.clear()

        for ti, j in enumerate(todo):
            flag, nt, q, _, long_way = jobs[j]
            gi = base + j
            save = list(cnt)
            fail = False
            if long_way:
                if run:
                    flush()
                tab_mask = None  # (the long way changes the mask behind the table's back: the next run tests for it)
                cmds, placed = [], 0
                if q == 0:
                    for t in range(nt):
                        q1 = qk[int(d["t_cls"][int(d["first"][gi]) + t])]
                        g = level_for(q1, mask(), spread) if 1 <= q1 <= 31 else 0
                        if not g:
                            fail = True; break
                        apply(g, g - q1, 1); cmds.append((g, max(g - q1, 0), 1, 1)); placed += 1
                else:
                    while placed < nt:
                        c = live_step(q, nt - placed)
                        if c is None:
                            fail = True; break
                        apply(c[0], c[1], c[2]); cmds.append(c[:4]); placed += c[2] * c[3]
                if fail:
                    cnt[:] = save
                else:
                    publish(cmds)
                last = (False, False)
            else:
                before = mask()
                if tab_mask != before:  # the kernel's test at a run's start and behind every gang: the table is rebuilt for the mask as it is
                    tab_mask = before; stats["rebuilds"] += 1
                word = table_word(q, nt, tab_mask, spread)
                first = live_step(q, nt)
                # the word is the live step but for the level's population
                assert (word is None) == (first is None), gi
                x = dict(q=q, before=before, emptied_top=False)
                stats["walked"] += 1
                if word is None:
                    fail = True; x.update(out="fail1", cmds=[], after=before)
                else:
                    g, g2, per, kq, whole = word
                    assert (g, max(g2, 0), per, kq) == (first[0], first[1], first[3], first[4]), (gi, word, first)
                    k = min(kq, cnt[g])
                    stats["steps"] += 1
                    if cnt[g] < kq:
                        found.add("i"); stats["clamped"] += 1
                    # (b), (c): what a table that was not rebuilt behind the run's earlier gangs would have said
                    if run:
                        p = run[-1]; pg = p.get("src")  # the previous gang emptied its level, which the word of a table built in front of it names for this gang too
                        if not spread and p["q"] == q and pg and pg != g and not (before >> pg) & 1 and level_for(q, p["before"], spread) == pg:
                            found.add("b")
                        for e in run:
                            if not spread and e.get("g2new") == g and q <= g and level_for(q, e["before"], spread) not in (0, g):
                                found.add("c")
                    apply(g, g2, k)
                    if spread and g == before.bit_length() - 1 and not cnt[g]:
                        x["emptied_top"] = True
                    first_after = mask()
                    x.update(src=g, g2new=g2 if g2 >= 1 and not (before >> g2) & 1 else None)
                    cmds, placed = [(g, max(g2, 0), k, per)], k * per
                    assert (placed == nt) == (whole and k == kq)
                    if placed < nt:
                        stats["second"] += 1; stats["steps"] += 1
                        c = live_step(q, nt - placed)
                        if c is None:
                            fail = True; cnt[:] = save
                            if first_after != before:
                                found.add("f")
                            x.update(out="fail2", cmds=[], after=before)
                        else:
                            apply(c[0], c[1], c[2]); cmds.append(c[:4]); placed += c[2] * c[3]
                            if placed < nt:
                                # a third step: the run ends in front of this gang, which goes the long way from the start (to the same end)
                                if any(y["after"] != y["before"] for y in run):
                                    found.add("g")
                                cnt[:] = save
                                flush()
                                tab_mask = None
                                cmds, placed = [], 0
                                while placed < nt:
                                    c = live_step(q, nt - placed)
                                    if c is None:
                                        fail = True; break
                                    apply(c[0], c[1], c[2]); cmds.append(c[:4]); placed += c[2] * c[3]
                                if fail:
                                    cnt[:] = save
                                else:
                                    publish(cmds)
                                x = None
                            else:
                                if mask() != first_after:
                                    found.add("e")
                                x.update(out="ok2", cmds=cmds, after=mask())
                    else:
                        x.update(out="ok1", cmds=cmds, after=first_after)
                if x is not None:
                    if x["after"] != x["before"]:
                        stats["flips"] += 1
                    wrong = (flag == BF_OK) == fail
                    if wrong and run and run[-1]["after"] != run[-1]["before"] and ti + 1 < len(todo) and not jobs[todo[ti + 1]][4]:
                        found.add("h")  # (short gangs of the same run stand behind it: the ones the kernel holds back and drops)
                    if ti == 0 and prev_last == (True, True):
                        found.add("k")
                    run.append(x)
                    last = (True, x["after"] != x["before"])
                else:
                    last = (False, False)
            assert d["out"][gi] == (BF_DEAD if fail else BF_OK), gi
            if (flag == BF_OK) == fail:
                mismatch, n_out = 1, j + 1
                break
        if run:
            flush()
        prev_last = last if todo and todo[-1] == jn - 1 and jn == 64 and not mismatch else None
        n_done = base + n_out
    assert (n_done, mismatch, commands) == (d["n_done"], d["mismatch"], d["commands"]), "the model of the counting machine does not describe this launch"
    assert [[int(x) for x in row] for row in d["words_out"]] == lv.words(d["LV"], d["NW"]), "the model of the levels' sets does not describe this launch"
    return found, stats


def write_launch(prefix, level_nodes, qs, jobs):
    """<prefix>.in in the dump's format: 256 nodes, level_nodes[g] = the nodes with g free devices; class c asks for qs[c] devices; jobs = (class, tasks, flag)"""
    LV, NW, C, Q = 8, 4, len(qs), 1
    words = np.zeros((LV, NW), np.uint64)
    for g, nodes in level_nodes.items():
        for n in nodes:
            words[g - 1, n >> 6] |= np.uint64(1 << (n & 63))
    V = len(jobs)
    nt = np.array([j[1] for j in jobs], np.int32)
    first = np.concatenate(([0], np.cumsum(nt)[:-1])).astype(np.int32)
    P = int(nt.sum())
    t_cls = np.repeat(np.array([j[0] for j in jobs], np.int32), nt)
    qd = np.zeros(64, np.float64); qd[:C] = qs
    with open(prefix + ".in", "wb") as f:
        f.write(struct.pack("<16i", 0x4b464c31, C, Q, P, V, LV, NW, 1, 0, NW, 0, 0, 0, 0, 0, 0))
        f.write(struct.pack("<8i", 256, 0, 0, 0, 0, 0, 0, 0))            # RoundParams: mode 0, from job 0
        f.write(struct.pack("<4i64b", LV, NW, 1, 0, *([-1] * 64)))       # BucketParams: no static class bitmaps
        f.write(qd.tobytes()); f.write(np.array([j[2] for j in jobs], np.uint8).tobytes())
        f.write(first.tobytes()); f.write(nt.tobytes()); f.write(np.array([j[0] for j in jobs], np.int32).tobytes())
        f.write(t_cls.tobytes()); f.write(words.tobytes())


# classes of the written launches: class c asks for QS[c] devices
QS = (1, 2, 4, 8)
C1, C2, C4, C8 = 0, 1, 2, 3


def launch_quiet(prefix):
    """(a), (k): 150 nodes with one free device, 10 with four.  Stretch 0: 64 gangs of one task of one device — the mask never changes.  Stretch 1: 63 more of them, and its last
    gang asks for two devices: a node of level 4 moves to level 2, which was empty.  Stretch 2's first gang asks for two devices and must take level 2."""
    jobs = [(C1, 1, BF_OK)] * 64 + [(C1, 1, BF_OK)] * 63 + [(C2, 1, BF_OK)] + [(C2, 1, BF_OK)] + [(C1, 1, BF_OK)] * 4
    write_launch(prefix, {1: range(0, 150), 4: range(150, 160)}, QS, jobs)
    return {"a", "k"}


def launch_changes(prefix):
    """(b) - (j), all in one run of one stretch (63 short jobs).  Level 1 holds 1 node, level 2 two, level 3 one, level 4 forty, level 8 two.
      jobs 0-1   two gangs of two devices empty level 2; job 2 (two devices) must take the next level, 3 — (b) — whose node goes to level 1;
      jobs 3-15  level 2 and 3 are empty: gangs of two devices alternate between level 4 (a node comes to level 2, which the next gang must take — (c)) and level 2 (emptied
                 again): with job 2, fourteen gangs that each change the mask — (d);
      job 16     three tasks of one device: level 1 holds two nodes (fewer than it wants — (i) — and emptied), its second step takes the one node of level 2, which is
                 emptied by a second step: (e);
      job 17     a whole node (8 devices); job 18, two whole nodes, predicted dead: the capacities at the stretch's start held two, now one is left — its first step empties
                 level 8, its second finds none and the rollback restores the mask: (f);
      job 19     the last whole node; jobs 20, 22: whole nodes, predicted dead, walked (level 8 held two at the stretch's start) — their word says "no level", between the
                 commits of jobs 19, 21 (two devices), 23 (four devices) — (j);
      job 24     levels 1 and 2 hold one node each by now: four tasks of one device need three steps — the run ends in front of it, behind all those changes: (g);
      jobs 25-   38 gangs of four devices, predicted to fit, where level 4 holds 30 nodes by then and nothing lies above it: the 30th empties the level and the 31st (job 55)
                 finds none — a misprediction directly behind a mask change, with seven short gangs of the same run behind it that must not be walked: (h)."""
    jobs = [(C2, 1, BF_OK)] * 4 + [(C2, 1, BF_OK)] * 12 + [(C1, 3, BF_OK)]
    jobs += [(C8, 1, BF_OK), (C8, 2, BF_DEAD), (C8, 1, BF_OK), (C8, 1, BF_DEAD), (C2, 1, BF_OK), (C8, 1, BF_DEAD), (C4, 1, BF_OK)]
    jobs += [(C1, 4, BF_OK)]
    jobs += [(C4, 1, BF_OK)] * 36 + [(C4, 1, BF_OK), (C4, 1, BF_OK)]
    write_launch(prefix, {1: [0], 2: [1, 2], 3: [3], 4: range(10, 50), 8: [60, 61]}, QS, jobs)
    return set("bcdefghij")


def written_cases(tmp, order):
    found = set()
    for name, write in (("quiet", launch_quiet), ("changes", launch_changes)):
        pre = os.path.join(str(tmp), f"{name}{order}")
        want = write(pre)
        r = subprocess.run([R.fill_replay(tmp), pre], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
        got, _ = walk(R.read_dump(pre))
        print(f"written launch '{name}', order {order}: cases {sorted(got)}")
        assert want <= got, f"the written launch '{name}' does not hold {sorted(want - got)}"
        if name == "changes":
            d = R.read_dump(pre)
            assert (d["n_done"], d["mismatch"]) == (56, 1) and d["V"] == 63, "job 55 ends the launch with seven jobs behind it"

        found |= got
    return found


_DUMPED = {}


def dumped_cases(name, tmp):
    """the cases the dumped launches of a snapshot hold (every launch over 1 000 planned jobs, walked by the model); the run itself against the oracle"""
    if name not in _DUMPED:
        pre = os.path.join(str(tmp), name.replace(".", "_"))
        snap, cfg = snapshot(name)
        os.environ["KAI_HOSTSIM_FILL_DUMP"] = pre
        try:
            res = HostSim.run(snap, cfg)
        finally:
            del os.environ["KAI_HOSTSIM_FILL_DUMP"]
        assert int(res.stats.reserved[7]) >> 32 == 1, "the fill did not run on k_fill_levels"
        ref = T.Oracle.run(snap, cfg)
        assert_same(res, ref)
        stats = lambda s: (s.decisions, s.jobs_attempted, s.jobs_committed, s.rollbacks)
        assert stats(res.stats) == stats(ref.stats)
        dumps = sorted(glob.glob(pre + "_*.in"))
        assert dumps, f"{name}: no launch over 1 000 planned jobs"
        found = set()
        for p in dumps:
            f, _ = walk(R.read_dump(p[:-3]), spread=name.endswith("spread"))
            found |= f
        print(f"{name}: {len(dumps)} launches, cases {sorted(found)}")
        _DUMPED[name] = (found, dumps)
    return _DUMPED[name]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_written_launches_hold_their_cases(order, tmp_path):
    assert written_cases(tmp_path, order) >= set("abcdefghijk")


def test_inputs_hold_every_case(tmp_path):
    """the model describes every dumped launch and every written one, and every case is held by some input; the snapshots the GPU test runs hold the cases it names"""
    union = written_cases(tmp_path, 0)
    for name in ("single_pods_800",) + tuple(GPU_INPUTS):
        found, _ = dumped_cases(name, tmp_path)
        assert GPU_INPUTS.get(name, set()) <= found, f"{name} does not hold {sorted(GPU_INPUTS.get(name, set()) - found)}: tests/test_gpu_fill_levels_table.py relies on it"
        assert "j" not in found, "a snapshot holds case j after all: the written launch is no longer needed for it"
        union |= found
    assert union == set(CASES), f"no input holds {sorted(set(CASES) - union)}"


@pytest.mark.parametrize("order", [0, 1, 2])
def test_dumped_launches_of_the_smallest_snapshot_replayed(order, tmp_path):
    """the bin-packed launches of config 5 at three hundredths through fill_replay: k_fill_levels, k_fill_counts and the scalar fill agree in every output and counter"""
    _, dumps = dumped_cases("c5_0.03_binpack", tmp_path)
    for p in dumps:
        r = subprocess.run([R.fill_replay(tmp_path), p[:-3]], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
