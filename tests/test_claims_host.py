"""The strip-claim arithmetic of the trace kernel (csrc/svo_sched.h: waves_starting_on, starting_rank, starting_counter,
claimed_entry, counter_has_entry, dealt_strip, dealt_place, dealt_length), driven on the host through tests/claims_driver.cpp.
The kernel calls these functions and nothing else to decide which strip a wave gets; if they disagree with each other a strip is
never traced, or traced twice, and nothing says so.  Held here: the no-schedule deal is a bijection between strips and (list,
entry) with the stated list lengths, and a list's reserved ranks plus its eight counters hand out every entry exactly once, the
probe's predicate being true exactly while a counter has one left."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "octree-tracer_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
SHARDS, SUBS, NONE = 8, 8, 0xFFFFFFFF
DEALS = list(range(301)) + [4093, 32400]
GRIDS = [1, 2, 7, 8, 9, 16, 17, 64, 257]  # workgroups, of four waves
WAVES = 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("claims") / "claims")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "claims_driver.cpp"), "-o", exe])
    return exe


def ask(driver, commands):
    return subprocess.run([driver], input="\n".join(commands) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()


@pytest.fixture(scope="module")
def deals(driver):
    """n_strips -> (lengths[8], lists[8] as dealt_strip says them up to 16 entries past the end, places[n] as dealt_place says)"""
    lines = iter(ask(driver, [f"deal {n}" for n in DEALS]))
    out = {}
    for n in DEALS:
        lengths, lists = [], []
        for l in range(SHARDS):
            tag, ll, length, *strips = next(lines).split()
            assert tag == "L" and int(ll) == l
            lengths.append(int(length))
            lists.append([int(s) for s in strips])
        tag, *flat = next(lines).split()
        assert tag == "P"
        out[n] = (lengths, lists, list(zip(map(int, flat[0::2]), map(int, flat[1::2]))))
    return out


def test_the_deal_puts_every_strip_in_exactly_one_entry(deals):
    for n, (lengths, lists, places) in deals.items():
        seen = sorted(s for lst in lists for s in lst if s != NONE)
        assert seen == list(range(n)), f"{n} strips: dealt {len(seen)}, {len(set(seen))} distinct"
        assert len(places) == n
        for s, (l, k) in enumerate(places):
            assert l < SHARDS and lists[l][k] == s, f"{n} strips: strip {s} is said to stand at list {l} entry {k}"


def test_the_stated_list_lengths_are_the_numbers_of_valid_entries(deals):
    for n, (lengths, lists, _) in deals.items():
        assert sum(lengths) == n
        for l in range(SHARDS):
            valid = [s != NONE for s in lists[l]]
            assert valid == [True] * lengths[l] + [False] * 17, f"{n} strips, list {l}: length {lengths[l]}, valid entries {sum(valid)}"
        # (equally long in strips up to one run: what the deal is for)
        assert max(lengths) - min(lengths) <= 16


def claim_cases(deals):
    lengths = set(range(201))
    for n in (4093, 32400, 300, 17):
        lengths.update(deals[n][0])
    return sorted(lengths)


def test_reserved_ranks_and_counters_hand_out_every_entry_once(driver, deals):
    lengths = claim_cases(deals)
    cases = [(length, blocks, l) for blocks in GRIDS for length in lengths for l in (0, (blocks - 1) % SHARDS, 7)]
    lines = iter(ask(driver, [f"claims {length} {blocks} {WAVES} {l}" for length, blocks, l in cases]))
    for length, blocks, l in cases:
        what = f"list {l} of {length} entries, {blocks} workgroups"
        tag, reserved = next(lines).split()
        assert tag == "R"
        reserved = int(reserved)
        tag, *starts = next(lines).split()
        ranks, counters = [int(v) for v in starts[0::2]], [int(v) for v in starts[1::2]]
        assert tag == "S" and sorted(ranks) == list(range(reserved)), f"{what}: the starting waves' ranks are {sorted(ranks)}"
        assert reserved == WAVES * len([b for b in range(blocks) if b % SHARDS == l]), what
        assert all(c < SUBS for c in counters)
        handed = [r for r in ranks if r < length]  # (more waves than entries: those waves look elsewhere)
        for j in range(SUBS):
            tag, jj, *rest = next(lines).split()
            assert tag == "C" and int(jj) == j
            bar = rest.index("|")
            mine = [int(v) for v in rest[:bar]]
            assert all(e < length for e in mine), f"{what}, counter {j}: hands out an entry past the end"
            handed += mine
            after = [int(v) for v in rest[bar + 1:]]
            for k, e, has in zip(after[0::3], after[1::3], after[2::3]):
                assert k >= len(mine) and e >= length and has == 0, f"{what}, counter {j}: answer {k} is entry {e}, has-entry {has}"
        assert sorted(handed) == list(range(length)), f"{what}: {len(handed)} entries handed out, {len(set(handed))} distinct"


def test_a_workgroup_starts_on_its_own_list_and_the_lists_counters_in_turn(driver):
    """workgroup b: list b % 8; the workgroups of a list start on its counters round-robin"""
    lines = ask(driver, [f"claims 100 64 {WAVES} {l}" for l in range(SHARDS)])
    for l in range(SHARDS):
        starts = lines[l * (2 + SUBS) + 1].split()[1:]
        counters = [int(v) for v in starts[1::2]]
        assert counters == [c for c in range(SUBS) for _ in range(WAVES)], (l, counters)


# ---- not claims: the timeline buffer's size, which the same kernel's instrumentation builds write by ----

def test_the_python_mirror_of_the_debug_buffer_constants(pkg):
    """octree-tracer_amd/gpu.py restates the header's SVO_DEBUG_* by hand: held to include/svo_hip.h"""
    import re
    header = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    waves = int(re.search(r"#define SVO_DEBUG_WAVES (\d+)u", header).group(1))
    row = int(re.search(r"#define SVO_DEBUG_ROW_WORDS (\d+)u", header).group(1))
    assert "#define SVO_DEBUG_BUFFER_WORDS (2u * SVO_DEBUG_WAVES * SVO_DEBUG_ROW_WORDS)" in header
    assert (pkg.gpu.DEBUG_WAVES, pkg.gpu.DEBUG_ROW_WORDS, pkg.gpu.DEBUG_BUFFER_WORDS) == (waves, row, 2 * waves * row)
