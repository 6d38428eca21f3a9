"""The strip schedule's device side, as far as it can be checked without a GPU: the share step (csrc/svo_sched.h:
balance_share_step, the arithmetic post_kernel's balance_step runs after it has reduced a frame's stamps) driven on the host
through tests/share_step_driver.cpp, the bound on a list's share that order_list_cap relies on, the list build of
tests/sched_ref.py under the most skewed shares the step reaches, and the restatement's own pieces on cases small enough to
check by eye (tests/test_sched_gpu.py holds the kernels to the restatement)."""
import os
import subprocess

import numpy as np
import pytest

import sched_ref as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "octree-tracer_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
FAST, SLOW = 1000.0, 4000.0  # mean list times (ticks) further apart than the 1.25 a step follows


def gain_of(update):
    return 0.6 if update <= 6 else 0.25  # post_kernel: large steps first


def fastest(n_fast, first=0):
    return [FAST if first <= k < first + n_fast else SLOW for k in range(8)]


def sequences():
    """name -> 16 updates of (frame time, the eight lists' mean times)"""
    seq = {"equal": [(5000, [3000.0] * 8)] * 16}
    for n in (1, 2, 3, 4):
        seq[f"fastest_{n}"] = [(5000, fastest(n))] * 16
        seq[f"fastest_{n}_last_lists"] = [(5000, fastest(n, 8 - n))] * 16
    seq["alternating"] = [(5000, fastest(4) if u % 2 else fastest(4, 4)) for u in range(16)]
    seq["one_fast_then_another"] = [(5000, fastest(1, 0 if u < 8 else 7)) for u in range(16)]
    # four lists pushed down to the lower clamp by the large steps, then one list alone fastest against a small sum of the rest
    seq["four_fast_then_one"] = [(5000, fastest(4) if u < 6 else fastest(1)) for u in range(16)]
    seq["four_slow_then_one_fast"] = [(5000, fastest(4, 4) if u < 5 else fastest(1)) for u in range(16)]
    # a frame time that keeps falling: the best shares are the ones of the frame before the restore
    seq["fastest_1_ever_faster"] = [(9000 - 100 * u, fastest(1)) for u in range(16)]
    # list 5 leaves no stamp on some frames: those updates step nothing
    seq["no_stamps"] = [(5000, [0.0 if (k == 5 and u in (2, 3, 9)) else t for k, t in enumerate(fastest(2))]) for u in range(16)]
    return seq


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shares") / "share_step")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, os.path.join(HERE, "share_step_driver.cpp"), "-o", exe])
    return exe


def run(driver, updates):
    """the balance words after each of `updates` (frame time, times), numbered from 1: rows of (shares[9], n_updates, best time, best shares[9])"""
    stdin = "".join(f"{u + 1} {gain_of(u + 1)} {t_last} " + " ".join(repr(float(t)) for t in T) + "\n" for u, (t_last, T) in enumerate(updates))
    out = subprocess.run([driver], input=stdin, capture_output=True, text=True, check=True).stdout
    rows = []
    for line in out.splitlines():
        a, b, c = line.split("|")
        rows.append(([int(v) for v in a.split()], *[int(v) for v in b.split()], [int(v) for v in c.split()]))
    assert len(rows) == len(updates)
    return rows


@pytest.fixture(scope="module")
def runs(driver):
    return {name: run(driver, updates) for name, updates in sequences().items()}


@pytest.mark.parametrize("name", list(sequences()))
def test_every_update_leaves_shares_the_list_cap_can_hold(runs, name):
    """bal[0] = 0, bal[8] = 65536, strictly increasing, and no list's share above 2/8: with it a list's part of a class of t
    strips is at most t / 4 + 1 after rounding, n / 4 + kCostClasses over the classes -- order_list_cap."""
    for u, (shares, *_rest) in enumerate(runs[name]):
        try:
            S.check_shares(shares)
        except AssertionError as e:
            raise AssertionError(f"{name}, update {u + 1}: {e}")


def test_equal_times_keep_equal_shares(runs):
    for shares, *_ in runs["equal"]:
        assert shares == [8192 * k for k in range(9)]


def test_persistently_fastest_lists_settle_below_a_quarter(runs):
    """A list that stays fastest is clamped to 1.6 eighths (13107.2) and renormalised against the rest.  With gain 0.6 the slow
    lists lose at most 12 % a step; for two fast lists of eight the fixed point of s = 13107.2 / (2 * 13107.2 + 0.88 (65536 - 2 s))
    is s = 14894 (0.2273), approached from below over the six large steps; the small steps (gain 0.25: 5 % a step) pull it back."""
    for n in (1, 2, 3, 4):
        rows = runs[f"fastest_{n}"]
        parts = [S.check_shares(r[0]) for r in rows[:15]]  # (update 16 restores)
        assert all(a[0] <= b[0] for a, b in zip(parts[:6], parts[1:6])) and parts[3][0] > parts[0][0], "a fastest list's share did not grow under the large steps"
        for u, p in enumerate(parts):
            assert min(p[:n]) > 8192 > max(p[n:]) and max(p) <= 14894 + 1, p
            # lists with equal times keep equal shares, up to the rounding of the cumulative fractions: one unit a share and update
            assert max(p[:n]) - min(p[:n]) <= 2 * (u + 1) and max(p[n:]) - min(p[n:]) <= 2 * (u + 1), p
    assert max(S.check_shares(r[0])[0] for r in runs["fastest_2"]) > 14500  # (and it does get close)


def test_a_list_without_stamps_steps_nothing(runs):
    rows = runs["no_stamps"]
    for u in (2, 3, 9):  # 0-based updates whose list 5 left no stamp
        assert rows[u][0] == rows[u - 1][0] and rows[u][1] == rows[u - 1][1], f"update {u + 1} stepped"
    assert rows[1][0] != rows[0][0] and rows[4][0] != rows[3][0]
    assert rows[-1][1] == 16 - 3


def test_update_16_restores_the_best_shares(runs):
    """keep-best notes the shares a frame was TRACED with when it beat every earlier one; update 16 puts them back"""
    rows = runs["fastest_1"]  # every frame took the same time: the first one's equal shares stay the best
    assert rows[-1][0] == [8192 * k for k in range(9)] and rows[-1][3] == rows[-1][0] and rows[-1][2] == 5000
    assert rows[-2][0] != rows[-1][0]
    rows = runs["fastest_1_ever_faster"]  # every frame beat the one before: the best shares are those update 15 left
    assert rows[-1][0] == rows[-2][0] and rows[-1][3] == rows[-2][0] and rows[-1][2] == 9000 - 1500
    assert rows[-1][1] == 16
    for before, row in zip(rows, rows[1:]):
        assert row[3] == before[0]  # noted before the step: the shares the frame was traced with


def most_skewed(runs):
    """the shares with the largest single share that any sequence reached"""
    return max((r[0] for rows in runs.values() for r in rows), key=lambda s: max(b - a for a, b in zip(s, s[1:])))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097, 32400])
def test_lists_fit_the_cap_under_the_most_skewed_shares(runs, n):
    shares = most_skewed(runs)
    assert max(b - a for a, b in zip(shares, shares[1:])) > 14000  # (skewed indeed)
    rng = np.random.default_rng(n)
    bpr = {4096: 64, 32400: 240}.get(n, 0)
    for what, classes in (("random classes", rng.integers(0, S.COST_CLASSES, n).astype(np.uint8)),
                          ("one class", np.full(n, 7, dtype=np.uint8)),
                          ("every class but a few strips", np.arange(n, dtype=np.uint32).astype(np.uint8) % S.COST_CLASSES)):
        lengths, lists = S.build_lists(classes, n, bpr, shares, S.list_cap(n))  # (raises beyond the cap)
        assert sorted(s for l in lists for s in l) == list(range(n)), what
        assert int(lengths.sum()) == n


def test_build_lists_refuses_what_the_cap_cannot_hold():
    shares = [0, 30000] + [30000 + 5076 * k for k in range(1, 8)]
    shares[8] = 65536
    with pytest.raises(OverflowError):
        S.build_lists(np.zeros(4096, dtype=np.uint8), 4096, 0, shares, S.list_cap(4096))


# ---- the restatement itself, by eye ----

def rec(steps):
    out = np.zeros(np.shape(steps), dtype=[("value", "<u4"), ("t", "<f4"), ("info", "<u4"), ("normal_bits", "<u4")])
    out["info"] = np.asarray(steps) | 0x10000  # (the hit bit: not a step)
    return out


def test_cost_classes_by_eye():
    # 20 x 9 pixels in 8 x 8 blocks: 3 x 2 blocks, the right column 4 wide, the bottom row 1 high
    steps = np.zeros((9, 20), dtype=np.uint32)
    steps[0, 0] = 3      # block 0: class 0
    steps[7, 7] = 4      # block 0 after all: class 1
    steps[3, 8] = 23     # block 1: class 5
    steps[7, 19] = 127   # block 2 (partial, its last pixel): class 31
    steps[8, 7] = 40     # block 3 (one row high): class 10
    steps[8, 16] = 255   # block 5: beyond the last class -> 31
    assert S.cost_classes(rec(steps), 3).tolist() == [1, 5, 31, 10, 0, 31]
    # the same pixels in 16 x 4 blocks, 2 x 3 of them: (0, 0) and (3, 8) share block 0, (7, 7) is in block 2, block 1 holds nothing
    assert S.cost_classes(rec(steps), 4).tolist() == [5, 0, 1, 31, 10, 31]
    # two rectangles, the second the first upside down (row r -> 8 - r: 40 and 4 in block 0, 23 in block 1, 127 and 255 in
    # block 2, the 3 alone in block 3): its blocks follow the first one's
    assert S.cost_classes(rec(np.stack([steps, steps[::-1]])), 3).tolist() == [1, 5, 31, 10, 0, 31, 10, 5, 31, 0, 0, 0]
    # shadow records add their steps per pixel before the maximum
    shadow = np.zeros_like(steps)
    shadow[3, 8] = 9     # 23 + 9 = 32: class 8
    shadow[0, 1] = 3     # alone in its pixel: block 0 keeps its 4
    assert S.cost_classes(rec(steps), 3, shadow=rec(shadow)).tolist() == [1, 8, 31, 10, 0, 31]
    # explicit rays: 64 a strip, the last strip ragged
    rays = np.zeros(130, dtype=np.uint32)
    rays[63], rays[64], rays[129] = 8, 12, 100
    assert S.cost_classes(rec(rays)).tolist() == [2, 3, 25]


def test_skip_classes_by_eye():
    skip = np.ones(130, dtype=np.uint8)
    assert S.skip_classes(skip, 130).tolist() == [255, 255, 255]
    skip[129] = 0  # the last strip holds one ray
    assert S.skip_classes(skip, 130).tolist() == [255, 255, 0]
    assert S.skip_classes(skip, 130, prev=np.array([4, 5, 6], dtype=np.uint8)).tolist() == [255, 255, 6]
    assert S.skip_classes(skip, 129).tolist() == [255, 255, 255]  # the ray lies behind the items
    skip[:] = 1
    skip[64] = 0
    assert S.skip_classes(skip, 130, prev=np.array([4, 5, 6], dtype=np.uint8)).tolist() == [255, 5, 255]
    assert S.skip_classes(skip[:128], 128).tolist() == [255, 0]


def test_danger_floor_by_eye():
    L = S.LONG_CLASS
    grid = np.array([[0, 0, 0, 0, 0],
                     [0, L, 0, 0, 9],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 31]], dtype=np.uint8)
    # radius 1, one long strip is enough, floor 8: the eight around (1, 1) and the three around (3, 4); 9 is above the floor
    want = np.array([[8, 8, 8, 0, 0],
                     [8, L, 8, 0, 9],
                     [8, 8, 8, 8, 8],
                     [0, 0, 0, 8, 31]], dtype=np.uint8)
    assert S.danger_floor(grid.reshape(-1), 5, 1, 1, 8).reshape(4, 5).tolist() == want.tolist()
    # two are needed: nowhere within radius 1; within radius 2 the column between them and (3, 2), (3, 3)
    assert S.danger_floor(grid.reshape(-1), 5, 1, 2, 8).tolist() == grid.reshape(-1).tolist()
    want2 = grid.copy()
    want2[:, 2:4] = 8
    want2[0, 2:4] = 0  # (rows 0: the 31 in row 3 is three rows away)
    assert S.danger_floor(grid.reshape(-1), 5, 2, 2, 8).reshape(4, 5).tolist() == want2.tolist()
    assert S.motion_option(0x1204) == (2, 1, 8)


def test_build_lists_by_eye():
    eq = [8192 * k for k in range(9)]
    # 16 strips of one class, equal shares: two a list, in strip order
    lengths, lists = S.build_lists(np.zeros(16, dtype=np.uint8), 16, 0, eq, 40)
    assert lengths.tolist() == [2] * 8 and lists == [[2 * k, 2 * k + 1] for k in range(8)]
    # the same on a 4 x 4 grid of blocks: column by column
    _, lists = S.build_lists(np.zeros(16, dtype=np.uint8), 16, 4, eq, 40)
    assert lists == [[0, 4], [8, 12], [1, 5], [9, 13], [2, 6], [10, 14], [3, 7], [11, 15]]
    # expensive classes first, 0xFF left out; bounds round to nearest: the 3 strips of a class are cut at 3 k / 8 = 0, 0.375,
    # 0.75, 1.125, 1.5, 1.875, 2.25, 2.625, 3 -> 0, 0, 1, 1, 2, 2, 2, 3, 3: one strip each for lists 1, 3 and 6
    classes = np.array([9, 255, 0, 9, 0, 255, 9, 0], dtype=np.uint8)
    lengths, lists = S.build_lists(classes, 8, 0, eq, 40)
    assert lists == [[], [0, 2], [], [3, 4], [], [], [6, 7], []] and lengths.tolist() == [0, 2, 0, 2, 0, 0, 2, 0]
    # shares: list 0 takes half of every class
    half = [0, 32768] + [32768 + 4681 * k for k in range(1, 7)] + [65536]
    _, lists = S.build_lists(np.array([1] * 4 + [0] * 4, dtype=np.uint8), 8, 0, half, 40)
    assert lists[0] == [0, 1, 4, 5]
