"""The static deal's rules (csrc/svo_deal.h) on the CPU: seed, step, keep-best, the "claims" verdict, the compare after a rebuild and
the host's per-frame plan, driven through tests/deal_driver.cpp -- the same functions svo_deal.hip runs as kernels, here as one
thread, with a model frame (a wave's time = its start delay + the costs of its strips) in place of the replay kernel.  Records do
not depend on the deal, so no other CPU test sees a change here; one scripted sequence is pinned in tests/golden/deal_table.txt."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "octree-tracer_amd", "csrc")
TABLE = os.path.join(GOLDEN, "deal_table.txt")
LEARN = 16  # kDealLearnFrames
CAP = 48    # entries reserved per list in these scripts


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deal") / "deal_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(os.path.dirname(os.path.abspath(__file__)), "deal_driver.cpp"), "-o", exe])
    return exe


def run(driver, script):
    return subprocess.run([driver], input="\n".join(script) + "\n", capture_output=True, text=True, check=True).stdout


def dumps(out):
    """every `dump` of a run: (state dict, {wave: [strips]})"""
    res, cur = [], None
    for line in out.splitlines():
        if line.startswith("state "):
            v = [int(x) for x in line.split()[1:]]
            cur = (dict(zip(("step", "best", "best_sample", "verdict", "seeds", "moves", "last_time", "last_moves", "claim_time"), v)), {})
        elif line.startswith("row "):
            assert "UNTERMINATED" not in line, line
            w, entries = line[4:].split(":")
            cur[1][int(w)] = [int(x) for x in entries.split()]
        elif line == "end":
            res.append(cur)
    return res


def lists_script(lengths, first=0):
    """8 lists of the given lengths over distinct strip numbers (list l: first + l, first + l + 8, ...): -> script lines, {l: strips}"""
    lines, strips = [], {}
    for l, n in enumerate(lengths):
        strips[l] = [first + l + 8 * k for k in range(n)]
        lines.append(f"list {l} {n} " + " ".join(str(s) for s in strips[l]))
    return lines, strips


def list_of_wave(w):
    return (w // 4) % 8


def check_partition(rows, strips, row_cap):
    """each strip of each list sits in exactly one row of a wave of that list; rows are shorter than row_cap"""
    seen = {l: [] for l in strips}
    for w, row in rows.items():
        assert len(row) < row_cap, (w, row)
        seen[list_of_wave(w)] += row
    for l in strips:
        assert sorted(seen[l]) == sorted(strips[l]), f"list {l}"


LENGTHS = [23, 10, 40, 17, 0, 31, 12, 36]  # uneven, one empty


def learn_script(grid, lengths, extra=(), steps=LEARN, claims_time=100000, per_frame=None):
    lines, strips = lists_script(lengths)
    script = [f"grid {grid} {CAP} 4"] + lines + list(extra) + [f"claims_time {claims_time}", "seed", "dump"]
    for k in range(steps):
        script += (per_frame(k) if per_frame else []) + ["frame", "step", "dump"]
    return script, strips


@pytest.mark.parametrize("grid", [8, 12, 20])  # 4 waves on every list; 8 on lists 0-3 and 4 on the rest; 12 and 8
def test_seed_and_steps_keep_every_strip_in_one_row_of_its_list(driver, grid):
    # some waves start late and some strips are dear, so the steps have something to move
    extra = [f"delay {w} {150 * (w % 5)}" for w in range(0, grid * 4, 3)] + [f"cost {s} {100 + 40 * (s % 7)}" for s in range(0, 330, 2)]
    script, strips = learn_script(grid, LENGTHS, extra)
    out = run(driver, script)
    row_cap = int(out.split()[1])
    assert row_cap >= 2 * max(-(-n // (4 * (grid // 8))) for n in LENGTHS) and row_cap & (row_cap - 1) == 0
    d = dumps(out)
    assert len(d) == LEARN + 1
    for st, rows in d:
        check_partition(rows, strips, row_cap)
    # the seed is the stratified deal: entry k of list l at position k div W of wave k mod W
    for w, row in d[0][1].items():
        l, rank = list_of_wave(w), (w // 32) * 4 + w % 4
        waves = ((grid + 7 - l) // 8) * 4
        assert row == strips[l][rank::waves], w
    assert d[-1][0]["moves"] > 0 and d[-1][0]["step"] == LEARN and d[-1][0]["verdict"] in (1, 2)
    assert d[0][0]["seeds"] == 1 and d[0][0]["claim_time"] == 100000


def test_equal_stamps_move_nothing(driver):
    lines, strips = lists_script(LENGTHS)
    script = ["grid 8 48 4"] + lines + ["seed", "dump"] + [f"stamp {w} 400 500" for w in range(32)] + ["step", "dump"]
    d = dumps(run(driver, script))
    assert d[0][1] == d[1][1] and d[1][0]["last_moves"] == 0 and d[1][0]["step"] == 1


def test_a_move_must_pay_for_itself_and_a_donor_keeps_a_strip(driver):
    lines, strips = lists_script([8, 4, 0, 0, 0, 0, 0, 0])  # list 0: two strips a wave (waves 0-3); list 1: one (waves 4-7)
    head = ["grid 8 48 2"] + lines + ["seed"]
    base = [f"stamp {w} 400 500" for w in range(32)]
    # wave 0 ends at 600, its last strip took 100 (began at 500); wave 1 ended at 520: the gap, 80, is less than the strip
    d = dumps(run(driver, head + base + ["stamp 0 500 600", "stamp 1 400 520", "step", "dump"]))
    assert d[0][0]["last_moves"] == 0
    # wave 1 ended at 480, before wave 0 began its last strip: the strip moves to the end of wave 1's row
    d = dumps(run(driver, head + base + ["stamp 0 500 600", "stamp 1 400 480", "step", "dump"]))
    assert d[0][0]["last_moves"] == 1 and d[0][1][0] == [0] and d[0][1][1] == [8, 40, 32]
    # list 1: wave 4 is as late against wave 5, but its strip is its only one
    d = dumps(run(driver, head + base + ["stamp 4 500 600", "stamp 5 400 480", "step", "dump"]))
    assert d[0][0]["last_moves"] == 0 and all(len(d[0][1][w]) == 1 for w in range(4, 8))


def test_a_late_wave_gives_strips_until_one_is_left(driver):
    script, strips = learn_script(8, [12] * 8, ["delay 0 5000"])  # wave 0 starts after all others have ended, every frame
    d = dumps(run(driver, script))
    assert [len(rows[0]) for st, rows in d[:4]] == [3, 2, 1, 1]
    for st, rows in d:
        check_partition(rows, strips, 32)


def test_keep_best_restores_the_best_table_the_seed_included(driver):
    # the seed's frame is the fastest: every later frame runs with a growing delay on one wave
    script, _ = learn_script(8, LENGTHS, ["delay 1 300"], per_frame=lambda k: [f"delay 9 {400 * k}"])
    d = dumps(run(driver, script))
    assert any(rows != d[0][1] for st, rows in d[1:-1])
    assert d[-1][1] == d[0][1] and d[-1][0]["best"] == d[1][0]["last_time"] == min(st["last_time"] for st, rows in d[1:])
    # the fastest frame comes in the middle: the table it was traced with comes back
    script, _ = learn_script(8, LENGTHS, ["delay 1 300"], per_frame=lambda k: [f"delay 9 {400 * abs(k - 6)}"])
    d = dumps(run(driver, script))
    times = [st["last_time"] for st, rows in d[1:]]  # frame k was traced with the table of dump k
    k_best = times.index(min(times))
    assert 0 < k_best < LEARN - 1 and d[-1][1] == d[k_best][1] and d[-1][0]["best"] == times[k_best]


@pytest.mark.parametrize("claims_time,learnt_time,verdict", [(100000, 0, 1), (100000, 200000, 1), (10, 0, 2), (100000, 10, 2)])
def test_verdict_is_claims_when_replay_never_beat_the_claiming_kernel(driver, claims_time, learnt_time, verdict):
    script, _ = learn_script(8, LENGTHS, [f"learnt_time {learnt_time}"], claims_time=claims_time)
    d = dumps(run(driver, script))
    assert [st["verdict"] for st, rows in d[:-1]] == [0] * LEARN and d[-1][0]["verdict"] == verdict
    # learning is over: another step changes nothing
    again = dumps(run(driver, script + ["frame", "step", "dump"]))
    assert again[-1] == again[-2]


def test_rebuilt_lists_keep_the_table_unless_they_differ(driver):
    script, strips = learn_script(8, LENGTHS, ["delay 0 900"])
    same, _ = lists_script(LENGTHS)
    d = dumps(run(driver, script + same + ["compare", "dump"]))
    assert d[-1] == d[-2] and d[-1][0]["seeds"] == 1
    other = list(same)
    other[2] = other[2].rsplit(" ", 1)[0] + " 999"  # the last entry of list 2
    d = dumps(run(driver, script + other + ["compare", "dump"]))
    assert d[-1][0]["seeds"] == 2 and d[-1][0]["step"] == 0 and d[-1][0]["verdict"] == 0 and d[-1][0]["claim_time"] == 100000
    strips[2][-1] = 999
    check_partition(d[-1][1], strips, 32)
    shorter = list(same)
    shorter[5] = f"list 5 {LENGTHS[5] - 1} " + " ".join(str(s) for s in strips[5][:-1])
    assert dumps(run(driver, script + shorter + ["compare", "dump"]))[-1][0]["seeds"] == 2


def test_rows_that_would_not_fit_stay_with_claims(driver):
    assert run(driver, ["grid 8 544 16"]).split() == ["row_cap", "0"]      # 2 048 strips on 8 workgroups: 136 a row
    assert run(driver, ["grid 4 48 16"]).split() == ["row_cap", "0"]       # lists without a wave
    assert run(driver, ["grid 1792 8132 16"]).split() == ["row_cap", "32"]  # the 1080p frame
    assert run(driver, ["grid 1792 32432 16"]).split() == ["row_cap", "128"]  # 4K
    assert run(driver, ["grid 4096 32432 16"]).split() == ["row_cap", "0"]  # more waves on a list than a step ranks


def plans(driver, frames):
    """policy lines: enabled plain stored at_rest balance_frames grid row_cap fresh seen_step seen_verdict rebuilt"""
    out = run(driver, ["policy " + " ".join(str(int(v)) for v in f) for f in frames])
    res = []
    for line in out.splitlines():
        t = line.replace("|", "").split()
        res.append({t[i]: int(t[i + 1]) for i in range(1, len(t), 2)})
    return res


def test_host_plan(driver):
    rest = (1, 1, 1, 1, 16, 1792, 32, 0, 0, 0, 0)
    learning = (1, 1, 1, 1, 9, 1792, 32, 0, 0, 0, 0)    # the list shares are still being learnt
    moved = (1, 1, 1, 0, 16, 1792, 32, 0, 0, 0, 0)
    p = plans(driver, [learning] + [rest] * (LEARN + 2))
    assert p[0]["replay"] == 0 and p[0]["seed"] == 0 and p[0]["seeded"] == 0
    assert [q["seed"] for q in p[1:]] == [1] + [0] * (LEARN + 1) and all(q["replay"] for q in p[1:])
    assert [q["step"] for q in p[1:]] == [1] * LEARN + [0, 0] and [q["mirror"] for q in p[1:]] == [0] * (LEARN - 1) + [1, 0, 0]
    # the verdict arrives: "claims" stops the replay, until the view changes and rests again
    p = plans(driver, [rest] * (LEARN + 1) + [rest[:7] + (1, 16, 2, 0)] + [rest] * 2 + [moved] + [rest] * 2)
    assert [q["replay"] for q in p] == [1] * (LEARN + 1) + [0, 0, 0] + [0] + [1, 1]
    assert p[LEARN + 1]["claims"] == 1 and p[LEARN + 4]["seeded"] == 0 and p[LEARN + 5]["seed"] == 1
    # the schedule's backstop rebuilds the lists of a resting view: one compare, steps again until the mirror shows none is needed
    p = plans(driver, [rest] * (LEARN + 1) + [rest[:7] + (1, 16, 1, 0)] + [rest[:10] + (1,)] + [rest] + [rest[:7] + (1, 16, 1, 0)] + [rest])
    assert [q["compare"] for q in p[LEARN + 1:]] == [0, 1, 0, 0, 0] and [q["seed"] for q in p[1:]] == [0] * (LEARN + 5)
    assert [q["step"] for q in p[LEARN + 1:]] == [0, 0, 1, 0, 0] and p[LEARN + 2]["mirror"] == 1 and p[-1]["learn_left"] == 0
    # anything that is not the plain resting frame drops the table; the option off does too
    for k, frame in enumerate([(0,) + rest[1:], (1, 0) + rest[2:], (1, 1, 0) + rest[3:], rest[:6] + (0,) + rest[7:]]):
        p = plans(driver, [rest, rest, frame, rest])
        assert [q["replay"] for q in p] == [1, 1, 0, 1] and p[2]["seeded"] == 0 and p[3]["seed"] == 1, k
    # another grid: seeded again
    p = plans(driver, [rest, rest, rest[:5] + (512, 16) + rest[7:]])
    assert [q["seed"] for q in p] == [1, 0, 1]


def golden_script():
    extra = [f"delay {w} {170 * (w % 4)}" for w in range(0, 48, 5)] + [f"cost {s} {90 + 35 * (s % 5)}" for s in range(0, 330, 3)]
    script, _ = learn_script(12, LENGTHS, extra, per_frame=lambda k: [f"delay 7 {60 * (k % 3)}"])
    same, _ = lists_script(LENGTHS)
    return script + same + ["compare", "dump"]


def test_scripted_sequence_matches_golden_table(driver):
    assert run(driver, golden_script()) == open(TABLE).read()
