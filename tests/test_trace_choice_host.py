"""Which kernel traces a frame, and with how many workgroups (csrc/svo_sched.h: kernel_kind, fuse_allowed, launch_choice,
replay_eligible, trace_slot, resident_workgroups, stack_grid_blocks), driven on the host through tests/trace_choice_driver.cpp.
svo_abi.cpp asks these functions and svo_kernels.hip launches what they say; nothing else decides.  Held here to a restatement
of the rules as they stood when each launch site still worked them out for itself: the kernel and its template arguments over the
whole cross product of what they depend on, one table slot per instantiation, and the grid arithmetic on the LDS sizes whose
measurements set the granule (profiles/r04_lds_granule_ab.log)."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "octree-tracer_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
RESTART, STACK = 0, 1
KIB = 1024


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trace_choice") / "trace_choice")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "trace_choice_driver.cpp"), "-o", exe])
    return exe


def ask(driver, commands):
    return subprocess.run([driver], input="\n".join(commands) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()


# ---- the choice ----

def expected_choice(variant, depth, pause, show_hits, misc, mode, count_rays, fuse_opt, debug_buf, replay_asked):
    """The rules, one line per site that used to state them."""
    want_stack = variant != RESTART and depth <= 22       # trace_launch: the top table is built for these
    debug_view = pause and show_hits                       # the view that reads counter bits: RESTART, nothing fused
    stack = want_stack and not debug_view
    fused = fuse_opt and want_stack and not debug_view     # fuse_shadow_rays and its two callers (sun direction in range)
    counting = (mode != 2 or count_rays) and not pause     # count_nodes, for either kernel
    shd = stack and fused                                  # shadow_hits
    dbg = stack and debug_buf and not shd                  # no timeline instantiation with fused shadows
    replay = replay_asked and stack and not counting and not shd and not debug_buf and not depth > 16  # deal_before: plain_static
    return dict(wanted=want_stack, fused=fused, stack=stack, ge=misc, deep=depth > 16, dbg=dbg, cnt=counting, shd=shd, replay=replay)


CROSS = list(itertools.product((RESTART, STACK), (1, 16, 17, 22, 23), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1)))


@pytest.fixture(scope="module")
def slots(driver):
    """(kTraceSlots, {(ge, deep, dbg, cnt, shd): slot} of the claiming instantiations, {ge: slot} of the replay twins)"""
    lines = ask(driver, ["slots"])
    assert lines[0].split()[0] == "N"
    claim, replay = {}, {}
    for line in lines[1:]:
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "S":
            claim[tuple(v[:5])] = v[5]
        else:
            assert tag == "R"
            replay[v[0]] = v[1]
    return int(lines[0].split()[1]), claim, replay


def test_every_launch_gets_the_kernel_the_rules_give_it(driver, slots):
    _, claim, _ = slots
    lines = ask(driver, ["choice " + " ".join(map(str, case)) for case in CROSS])
    assert len(lines) == len(CROSS)
    seen = set()
    for case, line in zip(CROSS, lines):
        tag, wanted, fused, _, stack, ge, deep, dbg, cnt, shd, replay, _, slot = line.split()
        assert tag == "K"
        want = expected_choice(*case)
        got = dict(wanted=int(wanted), fused=int(fused), stack=int(stack), cnt=int(cnt), shd=int(shd), dbg=int(dbg), replay=int(replay))
        if want["stack"]:  # (ge and deep pick no RESTART kernel)
            got.update(ge=int(ge), deep=int(deep))
        assert got == {k: int(bool(want[k])) for k in got}, f"{case}: {line}"
        if want["stack"]:
            key = (got["ge"], got["deep"], got["dbg"], got["cnt"], got["shd"])
            assert int(slot) == claim[key], f"{case}: slot {slot}, the table has {key} at {claim[key]}"
            seen.add(key + (got["replay"],))
    # the cross product reaches every instantiation: 24 claiming ones and the two replay twins
    assert {k[:5] for k in seen} == set(claim) and len([k for k in seen if k[5]]) == 2


def test_one_slot_per_instantiation_and_the_replay_twin_shares_its_default_twins(slots):
    n_slots, claim, replay = slots
    assert len(claim) == 24  # GE x deep x {plain, CNT, DBG, DBG CNT, SHD, SHD CNT}
    assert sorted(claim.values()) == sorted(set(claim.values())), "two instantiations share a slot"
    assert all(0 <= s < n_slots for s in claim.values())
    assert replay == {ge: claim[(ge, 0, 0, 0, 0)] for ge in (0, 1)}


# ---- the grid ----

def test_resident_workgroups_follow_the_lds_granule(driver):
    """the four measured sizes: the runtime's query does not round LDS up to the 1280-byte granule and says 8"""
    cases = [(22 * KIB + 512, 7), (22 * KIB + 528, 6), (26 * KIB, 6), (26 * KIB + 336, 5)]
    lines = ask(driver, [f"resident 8 {lds}" for lds, _ in cases])
    assert [int(line.split()[1]) for line in lines] == [n for _, n in cases]
    for lds, n in cases:  # (the rule itself: 160 KiB over the size rounded up to whole granules)
        assert n == 160 * KIB // (-(-lds // 1280) * 1280)


def test_a_runtime_answer_below_the_lds_bound_wins(driver):
    lines = ask(driver, [f"resident {rt} {22 * KIB + 512}" for rt in (5, 6, 7, 8, 1, 0)])
    assert [int(line.split()[1]) for line in lines] == [5, 6, 7, 7, 1, 1]  # (no answer counts as one workgroup)
    # more LDS than a CU has: the bound is below 1 and does not apply
    assert ask(driver, [f"resident 2 {161 * KIB}"]) == ["B 2"]


def expected_grid(cus, per_cu, override, debug_buf, n_items, strip_items):
    blocks = override if override > 0 else cus * per_cu
    if debug_buf:
        blocks = min(blocks, 16384 // 4)  # SVO_DEBUG_WAVES rows, four waves a workgroup
    n_strips = -(-n_items // strip_items)
    return min(blocks, -(-n_strips // 4))


GRIDS = [
    # cus, per CU, override, debug buffer, items, strip items -> workgroups
    ((256, 7, 0, 0, 1920 * 1080, 64), 1792),      # every CU full
    ((256, 7, 100, 0, 1920 * 1080, 64), 100),     # the override replaces the product ...
    ((256, 7, 6000, 0, 1920 * 1080, 64), 6000),   # ... above it too
    ((256, 7, 6000, 1, 1920 * 1080, 64), 4096),   # the debug buffer's cap
    ((1024, 7, 0, 1, 1920 * 1080, 64), 4096),
    ((256, 7, 4096, 1, 1920 * 1080, 64), 4096),
    ((256, 7, 0, 1, 1920 * 1080, 64), 1792),
    ((256, 7, 0, 0, 100000, 64), 391),            # 1563 strips: ceil(n_strips / 4)
    ((256, 7, 0, 0, 100000, 256), 98),            # 391 strips
    ((256, 7, 6000, 1, 100000, 256), 98),
    ((256, 7, 0, 0, 64 * 4 * 1792, 64), 1792),    # exactly enough strips
    ((256, 7, 0, 0, 64 * 4 * 1792 - 64, 64), 1792),
    ((256, 7, 0, 0, 64 * 4 * 1791, 64), 1791),
    ((256, 7, 0, 0, 1, 64), 1),                   # one ray: one workgroup
    ((256, 7, 0, 0, 1, 256), 1),
    ((256, 7, 0, 0, 257, 64), 2),                 # 5 strips
]


def test_the_grid_of_a_stack_launch(driver):
    lines = ask(driver, ["grid " + " ".join(map(str, case)) for case, _ in GRIDS])
    for (case, want), line in zip(GRIDS, lines):
        assert want == expected_grid(*case), case
        assert line == f"G {want}", f"{case}: {line}"
