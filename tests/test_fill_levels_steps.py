"""kai_fill_levels.hpp, the counting machine: a short gang that needs three and more steps stays in its run.

Up to KFL_HELD commands of a gang are held in lanes (c0 .. c2): a short gang that is not placed by its second step keeps walking out of line, inside the run, and the flush
stores every lane's commands one after the other — the task base of each the one before it plus k·per of the held word before it.  The state in front of the gang is kept once;
a later step that finds no level restores the counts and the mask from it, a misprediction at a later step ends the round there, a gang that needs more than KFL_HELD steps
leaves the run and goes the long way from the start.  The ring receives the words it received before, in the same order, so every output and counter stays what it was.

A model of the counting machine walks the INPUTS of launches written here in the dump's format (256 nodes, at most 200 jobs; the launch that reaches the ring's end needs 1 024 nodes: 256 hold 2 048 devices, fewer commands than the ring has slots) and of dumped launches (tests/host_sim,
KAI_HOSTSIM_FILL_DUMP), reproduces each launch's outcomes, its number of commands and the sets it leaves, and tells which of the cases below the launch holds.  A case that no
input holds fails the test.  The written launches are replayed by tests/host_sim/fill_replay.cpp — the emulated k_fill_levels and k_fill_counts against the scalar C++ fill, every
output and counter compared — under the three wavefront orders (kai_simt.hpp KW_EMU_ORDER), and so are the bin-packed dumped launches of config 5 at three hundredths.

Cases (a "multi-step gang": a short gang committed inside its run with three or more commands):
  three         a gang placed by exactly 3 steps
  held          a gang placed by exactly KFL_HELD steps
  long          a gang that needs KFL_HELD + 1 steps: it leaves the run and goes the long way
  rollback      a third or later step finds no level after steps that changed the mask: counts and mask are restored, and a gang of the same run behind it is walked
  fit_fails     a job predicted to fit fails at its third (or a later) step with short gangs of the same run behind it: the launch ends there
  dead_fits     a job predicted dead fits with three (or more) steps: the launch ends there
  lane63        a multi-step gang in lane 63
  stretch_last  a multi-step gang as a stretch's last job, the next stretch's first job walked in a run
  ring_end      a run of 64 gangs of KFL_HELD commands each, flushed across the ring's end
  behind        a multi-step gang directly behind another one in the run
"""
import collections
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import kai_testlib as T
import test_fill_levels_runs as R
import test_fill_levels_stretches as S
import test_fill_levels_table as M

BF_OK, BF_GATE, BF_DEAD = S.BF_OK, S.BF_GATE, S.BF_DEAD
KFL_SHORT, KFL_RING = S.KFL_SHORT, S.KFL_RING
with open(os.path.join(T.ROOT, "kai-scheduler_amd", "csrc", "kai_fill_levels.hpp")) as _f:
    KFL_HELD = int(re.search(r"constexpr int KFL_HELD = (\d+);", _f.read()).group(1))
CASES = ("three", "held", "long", "rollback", "fit_fails", "dead_fits", "lane63", "stretch_last", "ring_end", "behind")
# the snapshots of tests/test_gpu_fill_levels_steps.py and what each must hold (asserted below: the GPU test relies on it); under spread further steps are rare at these sizes:
# the spread snapshot is there for the spread instantiation of the same walk
GPU_INPUTS = {"c5_0.03_binpack": {"three"}, "c5_0.1_binpack": {"three", "behind"}, "c5_0.03_spread": set()}
THIRD_STEPS_AT_A_TENTH = 184  # the big round of config 5 at a tenth, bin-packed: short gangs that take a third step


def walk(d, spread=False, held=KFL_HELD):
    """The counting machine with up to `held` commands of a gang held in lanes, run by run; returns (cases the launch holds, counts for the write-up)."""
    LV, start, V = d["LV"], d["start"], d["V"]
    lv = R.Levels(d["words"])
    cnt = [0] + [len(lv.heap[g]) for g in range(1, LV + 1)]
    qk = [int(d["qd"][k]) for k in range(d["C"])]
    found = set()
    stats = collections.Counter()
    steps = collections.Counter()  # steps a walked short gang takes until it is placed or finds no level (the failing step counts)
    wp = commands = 0
    n_done, mismatch = start, 0
    prev_last = False  # the previous stretch's last job was a multi-step gang of a run

    def mask():
        return 1 | sum(1 << g for g in range(1, LV + 1) if cnt[g])

    def live_step(q, rem):
        g = M.level_for(q, mask(), spread)
        if not g:
            return None
        r = 1 if spread else max(g // q, 1)
        kq = max(rem if spread else rem // r, 1)
        per = min(r, rem)
        return g, max(g - per * q, 0), min(kq, cnt[g]), per

    def apply(c):
        cnt[c[0]] -= c[2]
        if c[1] >= 1:
            cnt[c[1]] += c[2]

    def publish(cmds):
        nonlocal commands, wp
        wp += len(cmds)
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
        wp += 1  # the stretch's marker
        stats["stretches"] += 1
        n_out = jn
        todo = [j for j, (flag, nt, q, is_def, _) in enumerate(jobs) if flag != BF_GATE and not is_def]
        run = []  # the run being walked, per gang: dict(ok, cmds, multi, rolled)
        last_multi = False

        def flush():
            stats["runs"] += 1
            cmds = [c for x in run if x["ok"] for c in x["cmds"]]
            if len(run) == 64 and all(x["ok"] and len(x["cmds"]) == held for x in run) and wp // KFL_RING != (wp + len(cmds) - 1) // KFL_RING:
                found.add("ring_end")
            for i, x in enumerate(run):
                if x["multi"] and i and run[i - 1]["multi"]:
                    found.add("behind")
                if x["rolled"] and i + 1 < len(run):
                    found.add("rollback")
            # (for the write-up: k gangs in a row that each change the mask cost k table rebuilds; were the table rebuilt only behind a gang that leaves the mask as it found it,
            # k - 1 of them would go and k gangs would take the general step instead of the table's)
            k = 0
            for x in run + [dict(flip=False)]:
                if x["flip"]:
                    k += 1
                else:
                    stats["streaks"] += 1 if k else 0; stats["streak_rebuilds_saved"] += max(k - 1, 0); stats["streak_general_steps"] += k if k > 1 else 0; k = 0
            publish(cmds)
            run.clear()

        for ti, j in enumerate(todo):
            flag, nt, q, _, long_way = jobs[j]
            gi = base + j
            save, before = list(cnt), mask()
            cmds, placed, fail = [], 0, False
            if q == 0:
                for t in range(nt):
                    q1 = qk[int(d["t_cls"][int(d["first"][gi]) + t])]
                    g = M.level_for(q1, mask(), spread) if 1 <= q1 <= 31 else 0
                    if not g:
                        fail = True; break
                    c = (g, max(g - q1, 0), 1, 1); apply(c); cmds.append(c); placed += 1
            else:
                while placed < nt:
                    c = live_step(q, nt - placed)
                    if c is None:
                        fail = True; break
                    apply(c); cmds.append(c); placed += c[2] * c[3]
            n = len(cmds) + (1 if fail else 0)
            changed = mask() != before
            if fail:
                cnt[:] = save
            in_run = not long_way and n <= held
            if not long_way:
                stats["walked"] += 1; steps[n] += 1
                if n == held + 1:
                    found.add("long")
            if in_run:
                multi = not fail and len(cmds) >= 3
                if multi:
                    found.add("three" if len(cmds) == 3 else "more")
                    if len(cmds) == held:
                        found.add("held")
                    if j == 63:
                        found.add("lane63")
                if ti == 0 and j == 0 and prev_last:
                    found.add("stretch_last")
                run.append(dict(ok=not fail, cmds=cmds, multi=multi, rolled=fail and n >= 3 and changed and flag == BF_DEAD, flip=not fail and changed))
                last_multi = multi and j == 63
            else:
                if run:
                    flush()
                if not fail:
                    publish(cmds)
                last_multi = False
            assert d["out"][gi] == (BF_DEAD if fail else BF_OK), gi
            if (flag == BF_OK) == fail:
                mismatch, n_out = 1, j + 1
                if in_run and n >= 3:
                    if fail and ti + 1 < len(todo) and not jobs[todo[ti + 1]][4]:
                        found.add("fit_fails")
                    if not fail:
                        found.add("dead_fits")
                break
        if run:
            flush()
        prev_last = last_multi and not mismatch
        n_done = base + n_out
    assert (n_done, mismatch, commands) == (d["n_done"], d["mismatch"], d["commands"]), "the model of the counting machine does not describe this launch"
    assert [[int(x) for x in row] for row in d["words_out"]] == lv.words(d["LV"], d["NW"]), "the model of the levels' sets does not describe this launch"
    found.discard("more")
    stats["third"] = sum(v for n, v in steps.items() if n >= 3)
    return found, stats, steps


def write_launch(prefix, level_nodes, qs, jobs, NW=4):
    """<prefix>.in in the dump's format: 64·NW nodes, level_nodes[g] = the nodes with g free devices; class c asks for qs[c] devices; jobs = (class, tasks, flag), or
    (tuple of classes, tasks, flag): a gang of several classes, its tasks taking the classes in turn"""
    LV, C, Q = 8, len(qs), 1
    words = np.zeros((LV, NW), np.uint64)
    for g, nodes in level_nodes.items():
        for n in nodes:
            words[g - 1, n >> 6] |= np.uint64(1 << (n & 63))
    V = len(jobs)
    nt = np.array([j[1] for j in jobs], np.int32)
    first = np.concatenate(([0], np.cumsum(nt)[:-1])).astype(np.int32)
    P = int(nt.sum())
    ucls = np.array([-1 if isinstance(j[0], tuple) else j[0] for j in jobs], np.int32)
    t_cls = np.concatenate([np.resize(np.array(j[0], np.int32), j[1]) for j in jobs]).astype(np.int32)
    qd = np.zeros(64, np.float64); qd[:C] = qs
    with open(prefix + ".in", "wb") as f:
        f.write(struct.pack("<16i", 0x4b464c31, C, Q, P, V, LV, NW, 1, 0, NW, 0, 0, 0, 0, 0, 0))
        f.write(struct.pack("<8i", 256, 0, 0, 0, 0, 0, 0, 0))            # RoundParams: mode 0, from job 0
        f.write(struct.pack("<4i64b", LV, NW, 1, 0, *([-1] * 64)))       # BucketParams: no static class bitmaps
        f.write(qd.tobytes()); f.write(np.array([j[2] for j in jobs], np.uint8).tobytes())
        f.write(first.tobytes()); f.write(nt.tobytes()); f.write(ucls.tobytes())
        f.write(t_cls.tobytes()); f.write(words.tobytes())


# classes of the written launches: class c asks for QS[c] devices
QS = M.QS
C1, C2, C4, C8 = M.C1, M.C2, M.C4, M.C8
# a gang of 16 tasks of one device that meets one node with four free devices and whole nodes behind it takes THREE steps — the node of level 4 (4 tasks), a whole node (8), and
# 4 tasks on the next whole node, which moves to level 4: the next such gang meets the same levels.
LADDER = (C1, 16, BF_OK)


def launch_ladder(prefix):
    """256 nodes: node 0 holds four free devices, nodes 64-255 eight.  Stretch 0 starts with two ladder gangs, one directly behind the other (three, held, behind).  Gangs of one
    and two devices then leave single nodes on the low levels, which gangs of 15 and 16 tasks of one device climb in three steps; job 9 meets a node at level 1 and one at
    level 6 in front of the whole nodes and needs FOUR steps — it leaves the run and goes the long way (long).  Jobs 10-13 bring the ladder's state back, ladder gangs and
    whole-node jobs alternate, and jobs 62 and 63 are ladder gangs (lane63, stretch_last: stretch 1 starts with a short gang).  Stretch 1's second job is predicted dead — the
    capacities at the stretch's start hold it, so it is walked — and fits with three steps (dead_fits): the launch ends there.  The model below tells what each gang really
    does; the test fails if the launch does not hold these cases."""
    jobs = [LADDER, LADDER, (C2, 1, BF_OK), (C1, 15, BF_OK), (C1, 15, BF_OK), (C1, 1, BF_OK), (C2, 1, BF_OK), (C1, 16, BF_OK), (C2, 1, BF_OK), (C1, 16, BF_OK)]
    jobs += [(C1, 12, BF_OK), (C1, 1, BF_OK), (C1, 2, BF_OK), (C4, 1, BF_OK)]  # level 7 + 5 of a whole node (-> level 3); level 3 -> 2; level 2 emptied; a whole node -> level 4: the ladder's state again
    jobs += [LADDER, (C8, 1, BF_OK)] * 24
    jobs += [LADDER, LADDER]
    assert len(jobs) == 64
    jobs += [(C1, 1, BF_OK), (C1, 16, BF_DEAD), (C1, 1, BF_OK), (C1, 1, BF_OK)]
    write_launch(prefix, {4: [0], 8: range(64, 256)}, QS, jobs)
    return {"three", "held", "long", "behind", "lane63", "stretch_last", "dead_fits"}


def launch_rollback(prefix):
    """256 nodes: level 1 ten nodes, level 2 one, level 4 one, level 5 one, level 8 one.  Job 0 takes the whole node.  Job 1, three tasks of four devices, predicted dead, is walked
    (the capacities at the stretch's start hold four such tasks): level 4 and level 5 take one each and are emptied, the third step finds no level — the rollback restores both
    levels and the mask, and job 2 (four devices) behind it, in the same run, must take level 4 again (rollback).  Job 3, eight tasks of two devices predicted to fit: level 2, then
    level 5 (two of them), and no level for its third step (fit_fails): the launch ends there, the five short gangs behind it are not walked."""
    jobs = [(C8, 1, BF_OK), (C4, 3, BF_DEAD), (C4, 1, BF_OK), (C2, 8, BF_OK)] + [(C1, 1, BF_OK)] * 5
    write_launch(prefix, {1: range(10, 20), 2: [3], 4: [0], 5: [1], 8: [2]}, QS, jobs)
    return {"rollback", "fit_fails"}


def launch_ring_end(prefix):
    """1 024 whole nodes.  Stretch 0: four gangs of two classes with 975, 975, 975 and 978 tasks, task by task — 3 903 commands, which leave one node at level 4 and whole nodes —
    and 60 whole-node jobs.  Stretch 1: 64 ladder gangs, one run of 64 x KFL_HELD = 192 commands flushed from slot 3 965 on: across the ring's end at 4 096 (ring_end)."""
    assert KFL_HELD == 3, "the ladder gang takes three steps: another KFL_HELD needs another gang here"
    several = (C1, C1, C2, C1, C1, C1, C1)  # seven tasks, eight devices: a whole node
    jobs = [(several, 975, BF_OK)] * 3 + [(several, 978, BF_OK)] + [(C8, 1, BF_OK)] * 60 + [LADDER] * 64
    write_launch(prefix, {8: range(0, 1024)}, QS, jobs, NW=16)
    return {"ring_end", "behind", "lane63", "three", "held"}


LAUNCHES = (("ladder", launch_ladder), ("rollback", launch_rollback), ("ring_end", launch_ring_end))


def written_cases(tmp, order):
    found = set()
    for name, write in LAUNCHES:
        pre = os.path.join(str(tmp), f"{name}{order}")
        want = write(pre)
        r = subprocess.run([R.fill_replay(tmp), pre], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
        d = R.read_dump(pre)
        got, stats, steps = walk(d)
        print(f"written launch '{name}', order {order}: cases {sorted(got)}, steps per walked gang {dict(sorted(steps.items()))}")
        assert want <= got, f"the written launch '{name}' does not hold {sorted(want - got)}"
        if name == "rollback":
            assert (d["n_done"], d["mismatch"], d["V"]) == (4, 1, 9), "job 3 ends the launch with five jobs behind it"
            assert [int(x) for x in d["out"][:4]] == [BF_OK, BF_DEAD, BF_OK, BF_DEAD]
        found |= got
    return found


def dumped(name, tmp):
    """the dumped launches of a snapshot (made, and held against the oracle, by tests/test_fill_levels_table.py's helper) walked by this module's model: (cases, per launch
    the gangs that take a third step, the dumps)"""
    _, dumps = M.dumped_cases(name, tmp)
    found, third = set(), []
    for p in dumps:
        f, stats, _ = walk(R.read_dump(p[:-3]), spread=name.endswith("spread"))
        found |= f; third.append(stats["third"])
    print(f"{name}: {len(dumps)} launches, cases {sorted(found)}, gangs with a third step per launch {third}")
    return found, third, dumps


@pytest.mark.parametrize("order", [0, 1, 2])
def test_written_launches_hold_their_cases(order, tmp_path):
    """every case is held by a written launch, whose replay agrees with the scalar fill and k_fill_counts in every output and counter"""
    found = written_cases(tmp_path, order)
    assert found == set(CASES), f"no written launch holds {sorted(set(CASES) - found)}"


@pytest.mark.parametrize("name", tuple(GPU_INPUTS))
def test_gpu_inputs_hold_their_cases(name, tmp_path):
    """the model describes every dumped launch of the snapshots the GPU test runs, and they hold the cases it names (every case is held by a written launch: the test above)"""
    found, third, _ = dumped(name, tmp_path)
    assert GPU_INPUTS[name] <= found, f"{name} does not hold {sorted(GPU_INPUTS[name] - found)}: tests/test_gpu_fill_levels_steps.py relies on it"
    assert found <= set(CASES)
    if name == "c5_0.1_binpack":
        assert max(third) == THIRD_STEPS_AT_A_TENTH, third


@pytest.mark.parametrize("order", [0, 1, 2])
def test_dumped_launches_of_the_smallest_snapshot_replayed(order, tmp_path):
    """the bin-packed launches of config 5 at three hundredths hold third steps, and through fill_replay k_fill_levels, k_fill_counts and the scalar fill agree in every output
    and counter"""
    _, third, dumps = dumped("c5_0.03_binpack", tmp_path)
    assert sum(third) > 0, "no gang of these launches takes a third step"
    for p in dumps:
        r = subprocess.run([R.fill_replay(tmp_path), p[:-3]], env=dict(os.environ, KW_EMU_ORDER=str(order), KW_EMU_SEED="23"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr[-2000:]
