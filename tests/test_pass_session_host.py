"""What makes the pass sessions (tests/test_pass_session_gpu.py) worth running, held on the host: the restatements agree with
each other on the composed inputs the GPU will see -- after every mutating op the model's words, sampled over the whole grid,
equal a dense grid that only the per-cell contracts update -- and the seeded sessions and worst_transitions() together put every
pass directly behind every mutating pass and behind every refusal of a pass it shares a workspace with, cross a scan tile and
drop back under it, feed the passes layouts no builder made, and rest long enough for the static deal before writes of every
kind.  Without these conditions the GPU test could pass while checking nothing.  The tallies are printed (-s shows them).

The same for the second table (tests/pass_session_ops2.py: combine, rects, components and drop; the sessions seed301..seed303
and worst_combinations()), on its own sessions: every new pass directly behind every mutating pass, every pass directly behind
a combine and a drop that drops, every new refusal kind directly before each partner, the sizes, the layouts, all six combine
ops and three source forms, drops that drop nothing, some and all, and the rests of worst_combinations() as the Tracker plans
them.  The seven sessions of the first table are pinned to their op lines (tests/golden/pass_session_ops.txt): a name added to
its tables would reshuffle them without a test noticing."""
import collections

import os

import numpy as np
import pytest

import pass_session_ops as P
import pass_session_ops2 as P2
import session_ops as S
from conftest import GOLDEN


@pytest.fixture(scope="module")
def sessions(pkg):
    return {name: P.session(name) for name in P.NAMES}


@pytest.fixture(scope="module")
def plans(O, sessions, tmp_path_factory):
    """name -> the owner's frames as session_ops.Tracker sees them, every launch with the policy's row and the deal's facts"""
    driver = S.build_driver(tmp_path_factory.mktemp("pass_session_plan"))
    return {name: S.Tracker(P.Views(O)).plan(P.owner_ops(steps)[0], driver) for name, steps in sessions.items()}


def neighbours(steps):
    """(the (mutating pass, pass) pairs and the (refusal kind, pass) pairs that stand side by side)"""
    pairs, after_refusal = collections.Counter(), collections.Counter()
    last = refusal = None
    for s in steps:
        if s["op"].kind == "frame":
            last = refusal = None
        elif s["refused"]:
            last, refusal = None, s["op"].args[0]
        else:
            for k, call in enumerate(s["calls"]):
                if last is not None:
                    pairs[(last, call)] += 1
                if refusal is not None:
                    after_refusal[(refusal, call)] += 1
                refusal = None
                last = call if s["mutates"] and k == len(s["calls"]) - 1 else None
    return pairs, after_refusal


def test_sessions_are_deterministic_and_one_line_per_op(pkg, sessions):
    again = P.make_session(pkg, P.SEEDS[0], P.all_pairs()[0::len(P.SEEDS)], P.all_refusal_pairs()[0::len(P.SEEDS)])
    first = sessions[P.NAMES[0]]
    assert [s["op"] for s in again] == [s["op"] for s in first]
    assert all(a["words"] is None and b["words"] is None or np.array_equal(a["words"], b["words"]) for a, b in zip(again, first))
    for name, steps in sessions.items():
        assert all("\n" not in repr(s["op"]) and len(repr(s["op"])) < 120 for s in steps), name
        print(f"{name}: {dict(P.tallies(steps))}")
    assert len(P.SEEDS) == 6 and len(set(P.SEEDS)) == 6
    for seed in P.SEEDS:
        assert 80 <= len(sessions[f"seed{seed}"]) <= 160, (seed, len(sessions[f"seed{seed}"]))


def test_words_against_cells(sessions):
    """the restatements held to each other: build_ref, edit_ref, region_ref, compact_ref and simplify_ref make the words,
    region_ref.apply_cells, the edit's per-cell rule and simplify_ref.cut_cells make the grid, sample_ref compares them"""
    compared = 0
    for name, steps in sessions.items():
        for i, s in enumerate(steps):
            if s["mutates"]:
                differ, finer = s["cells_differ"]
                assert differ == 0, f"{name}, op {i}: {s['op']!r}: {differ} cells of the words differ from the per-cell contracts' grid"
                assert finer == 0, f"{name}, op {i}: {s['op']!r}: {finer} cells sample FINER, and the model holds no tree finer than its grid"
                compared += 1 << (3 * s["depth"])
            assert s["high"] <= P.CAPACITY and s["length"] <= s["high"], f"{name}, op {i}: over the capacity"
            assert s["declared"] == P.DECLARED
    print(f"cells compared: {compared}")
    assert compared > 10_000_000


def test_every_pass_directly_behind_every_mutating_pass_and_every_refusal(sessions):
    pairs, after_refusal = collections.Counter(), collections.Counter()
    for steps in sessions.values():
        a, b = neighbours(steps)
        pairs.update(a)
        after_refusal.update(b)
    missing = [p for p in P.all_pairs() if not pairs[p]]
    assert not missing, f"never side by side: {missing}"
    missing = [p for p in P.all_refusal_pairs() if not after_refusal[p]]
    assert not missing, f"never directly behind the refusal: {missing}"
    assert len(P.all_pairs()) == 7 * 13
    print(f"pairs (mutating pass, pass): {len(P.all_pairs())} of {len(P.all_pairs())}, fewest {min(pairs[p] for p in P.all_pairs())} times; "
          f"(refusal, pass): {len(P.all_refusal_pairs())}, fewest {min(after_refusal[p] for p in P.all_refusal_pairs())} times")
    kinds = collections.Counter(s["op"].args[0] for steps in sessions.values() for s in steps if s["refused"])
    print(f"refusals: {dict(kinds)}")
    assert set(kinds) == set(P.REFUSALS)
    via = collections.Counter(s["calls"][-1] for steps in sessions.values() for s in steps if s["mutates"] and s["via"])
    print(f"writes through the sharing context: {dict(via)}")
    assert set(via) == set(P.MUTATING)


def test_sizes_cross_a_scan_tile_and_drop_back(sessions):
    """each pass sees an input of more than 4 096 groups and, later in the same session, one of fewer than 512"""
    both = collections.Counter()
    for steps in sessions.values():
        large = set()
        for s in steps:
            for call in s["calls"]:
                if s["groups_in"] > P.TILE:
                    large.add(call)
                elif s["groups_in"] < P.SMALL and call in large:
                    both[call] += 1
    print(f"large, then small on one context: {dict(both)}")
    assert set(both) == set(P.PASSES), set(P.PASSES) - set(both)
    most = max(s["high"] for steps in sessions.values() for s in steps)
    print(f"the longest tree: {most} words of {P.CAPACITY}")


def test_layouts_no_builder_made(sessions):
    """compact, simplify, list, surface, sample and tops each meet a non-canonical layout at least three times; one tree holds
    a leaf of every level from 2 to its depth"""
    odd = collections.Counter()
    for steps in sessions.values():
        for s in steps:
            if s["canonical_in"] is False:
                odd.update(set(s["calls"]) - {"structure", "edit"})
    print(f"non-canonical inputs: {dict(odd)}")
    for name in ("compact", "simplify", "list", "surface", "sample", "tops"):
        assert odd[name] >= 3, (name, odd[name])
    every = [s for steps in sessions.values() for s in steps if s["levels"] and set(range(2, s["depth"] + 1)) <= set(s["levels"])]
    print(f"trees with a leaf of every level from 2 to their depth: {len(every)}")
    assert every


def test_rests_before_writes_of_every_kind(sessions, plans, O):
    """a 34-frame rest of the owner directly before an edit, a region edit, a compaction and a simplification in place, a build,
    a write through the sharing context and an out-of-place simplification; the frames of the rest are replayed, the first frame
    behind an in-place write is not, and the out-of-place simplification of worst_transitions stands between two frames that
    must be replayed"""
    assert not S.culls(P.Views(O).uniforms(P.REST_POSE), 2), "the resting pose is culled: the deal would never replay"
    seen = collections.Counter()
    must = collections.Counter()
    for name, steps in sessions.items():
        frames_of, k = [], 0
        for n in P.owner_ops(steps)[1]:
            frames_of.append(plans[name][k:k + n])
            k += n
        assert k == len(plans[name])
        for i, s in enumerate(steps[:-1]):
            if s["op"] != S.Op("frame", P.REST_POSE, 34):
                continue
            replay = [F["launches"][0]["replay"] for F in frames_of[i]]
            # (DEAL_LEARN of them where the view is new; fewer where frames of the same view and tree stood before the rest)
            assert replay.count(1) >= S.DEAL_LEARN // 2, f"{name}, op {i}: the rest replays {replay.count(1)} frames for certain"
            must["frames of a rest that must be replayed"] += replay.count(1)
            nxt = steps[i + 1]
            after = next((f for f in frames_of[i + 1:] if f), None)
            if nxt["mutates"]:
                kind = "build" if nxt["calls"][-1].startswith("build") else nxt["calls"][-1]
                seen[kind] += 1
                seen["through the sharing context"] += nxt["via"]
                assert after is not None and after[0]["launches"][0]["replay"] == 0, f"{name}, op {i + 1}: a replay straight after a write"
            elif nxt["op"].kind == "simplify":
                seen["out of place"] += 1
                assert after is not None and after[0]["launches"][0]["replay"] != 0, f"{name}, op {i + 1}: an out-of-place call ends the rest"
        for i, s in enumerate(steps[1:-1], 1):
            if s["op"].kind == "simplify" and not s["mutates"] and frames_of[i - 1] and frames_of[i + 1]:
                if frames_of[i - 1][-1]["launches"][0]["replay"] == 1 and frames_of[i + 1][0]["launches"][0]["replay"] == 1:
                    must["out-of-place simplifications between two frames that must be replayed"] += 1
    print(f"a 34-frame rest directly before: {dict(seen)}; {dict(must)}")
    for kind in ("edit", "region", "compact", "simplify", "build", "through the sharing context", "out of place"):
        assert seen[kind], kind
    assert must["out-of-place simplifications between two frames that must be replayed"] >= 1


# ---- the first table's sessions, pinned ----

def test_the_first_tables_sessions_keep_their_op_lines(sessions):
    with open(os.path.join(GOLDEN, "pass_session_ops.txt")) as f:
        want = f.read().splitlines()
    got = [f"{name} {i}: {s['op']!r}" for name in P.NAMES for i, s in enumerate(sessions[name])]
    assert len(got) == len(want), f"{len(got)} ops, {len(want)} pinned"
    moved = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not moved, f"{len(moved)} op lines moved, the first: got {got[moved[0]]!r}, pinned {want[moved[0]]!r}"
    assert P.NAMES == ("seed201", "seed202", "seed203", "seed204", "seed205", "seed206", "worst_transitions")
    assert not set(P2.PASSES2) & set(P.PASSES) and not set(P2.REFUSALS2) & set(P.REFUSALS)


# ---- the second table ----

@pytest.fixture(scope="module")
def sessions2(pkg):
    return {name: P2.session(name) for name in P2.NAMES2}


@pytest.fixture(scope="module")
def plans2(O, sessions2, tmp_path_factory):
    driver = S.build_driver(tmp_path_factory.mktemp("pass_session_plan2"))
    return {name: S.Tracker(P.Views(O)).plan(P.owner_ops(steps)[0], driver) for name, steps in sessions2.items()}


def test_new_sessions_are_deterministic_and_one_line_per_op(pkg, sessions2):
    P2.session.cache_clear()
    again = P2.session(P2.NAMES2[0])
    first = sessions2[P2.NAMES2[0]]
    assert [s["op"] for s in again] == [s["op"] for s in first]
    assert all(a["words"] is None and b["words"] is None or np.array_equal(a["words"], b["words"]) for a, b in zip(again, first))
    for name, steps in sessions2.items():
        assert all("\n" not in repr(s["op"]) and len(repr(s["op"])) < 120 for s in steps), name
        assert 45 <= len(steps) <= 90, (name, len(steps))
        print(f"{name}: {dict(P.tallies(steps))}")
    assert P2.ALL_NAMES == P.NAMES + P2.NAMES2 and len(P2.ALL_NAMES) == 11


def test_new_words_against_cells(sessions2):
    """as test_words_against_cells, with combine_ref.combine making the words and combine_ref.apply_cells the grid, and
    components_ref.drop_floating on the grid against components_ref.labels on the words"""
    compared = 0
    for name, steps in sessions2.items():
        for i, s in enumerate(steps):
            if s["mutates"]:
                differ, finer = s["cells_differ"]
                assert differ == 0, f"{name}, op {i}: {s['op']!r}: {differ} cells of the words differ from the per-cell contracts' grid"
                assert finer == 0, f"{name}, op {i}: {s['op']!r}: {finer} cells sample FINER, and the model holds no tree finer than its grid"
                compared += 1 << (3 * s["depth"])
            assert s["high"] <= P.CAPACITY and s["length"] <= s["high"], f"{name}, op {i}: over the capacity"
            assert s["declared"] == P.DECLARED
    combines = sum(s["op"].kind == "combine" for steps in sessions2.values() for s in steps)
    print(f"cells compared: {compared}, behind {combines} combines")
    assert compared > 4_000_000 and combines >= 40


def test_new_passes_directly_behind_every_mutating_pass_and_every_refusal(sessions2):
    pairs, after_refusal = collections.Counter(), collections.Counter()
    for steps in sessions2.values():
        a, b = neighbours(steps)
        pairs.update(a)
        after_refusal.update(b)
    # every new pass behind every mutating pass, old and new; every pass behind a combine and behind a drop that drops
    want = [(a, b) for a in P2.ALL_MUTATING for b in P2.PASSES2] + [(a, b) for a in P2.MUTATING2 for b in P2.ALL_PASSES]
    assert set(want) == set(P2.all_pairs2()) and len(set(want)) == 9 * 4 + 2 * 17 - 2 * 4
    missing = [p for p in P2.all_pairs2() if not pairs[p]]
    assert not missing, f"never side by side: {missing}"
    missing = [p for p in P2.all_refusal_pairs2() if not after_refusal[p]]
    assert not missing, f"never directly behind the refusal: {missing}"
    missing = [p for p in P2.old_refusal_pairs2() if not after_refusal[p]]
    assert not missing, f"never directly behind the first table's refusal: {missing}"
    assert {("max_words_region", "combine"), ("malformed_surface", "rects"), ("malformed_list", "components")} <= set(P2.old_refusal_pairs2())
    for kind, (p, _, _) in P2.REFUSALS2.items():
        assert p in P2.partners2(kind), kind  # (a successful call of the same pass directly behind its refusal)
    for a, b in (("combine", "region"), ("combine", "edit"), ("combine", "build"), ("rects", "surface"), ("components", "list")):
        assert any(a in group and b in group for group in P2.SHARED2.values()), (a, b)
    print(f"pairs (mutating pass, pass): {len(P2.all_pairs2())}, fewest {min(pairs[p] for p in P2.all_pairs2())} times; "
          f"(refusal, pass): {len(P2.all_refusal_pairs2())}, fewest {min(after_refusal[p] for p in P2.all_refusal_pairs2())} times")
    kinds = collections.Counter(s["op"].args[0] for steps in sessions2.values() for s in steps if s["refused"])
    print(f"refusals: {dict(kinds)}")
    assert set(P2.REFUSALS2) <= set(kinds)
    via = collections.Counter(s["calls"][-1] for steps in sessions2.values() for s in steps if s["mutates"] and s["via"])
    print(f"writes through the sharing context: {dict(via)}")
    assert set(P2.MUTATING2) <= set(via)


def test_new_sizes_cross_a_scan_tile_and_drop_back(sessions2):
    """each new pass sees an input of more than 4 096 groups and, later in the same session, one of fewer than 512"""
    both = collections.Counter()
    for steps in sessions2.values():
        large = set()
        for s in steps:
            for call in s["calls"]:
                if s["groups_in"] > P.TILE:
                    large.add(call)
                elif s["groups_in"] < P.SMALL and call in large:
                    both[call] += 1
    print(f"large, then small on one context: {dict(both)}")
    assert set(P2.PASSES2) <= set(both), set(P2.PASSES2) - set(both)


def test_new_passes_meet_layouts_no_builder_made(sessions2):
    """each new pass meets a non-canonical layout at least three times; rects meets a tree of mixed levels with rounds > 1"""
    odd = collections.Counter()
    for steps in sessions2.values():
        for s in steps:
            if s["canonical_in"] is False:
                odd.update(s["calls"])
    print(f"non-canonical inputs: {dict(odd)}")
    for name in P2.PASSES2:
        assert odd[name] >= 3, (name, odd[name])
    mixed = [s for steps in sessions2.values() for s in steps if s["op"].kind == "rects" and s["op"].args[2] > 1 and s["action"]["levels"] > 1]
    print(f"rects with rounds > 1 on a tree of mixed levels: {len(mixed)}")
    assert mixed


def test_combines_and_drops_of_every_kind(sessions2):
    ops, forms, trees, placed, drops, anchors = (collections.Counter() for _ in range(6))
    for steps in sessions2.values():
        for s in steps:
            op = s["op"]
            if op.kind == "combine":
                ops[op.args[0]] += 1
                forms[s["action"]["form"]] += 1
                trees[op.args[1].split("/")[1].rstrip("0123456789")] += 1
                placed[min(op.args[2], 1)] += 1
                assert all(0 <= v < 1 << op.args[2] for v in op.args[3])
            elif op.kind == "drop":
                n, dropped, leaves = s["want"]["triple"]
                assert s["mutates"] == (leaves > 0) == (s["writes"] == 1) and (dropped > 0) == (leaves > 0)
                drops["nothing" if not dropped else "all" if dropped == n else "some"] += 1
                anchors["floor" if op.args[0] is None else "box"] += 1
    print(f"combine ops: {dict(ops)}; sources: {dict(forms)} of {dict(trees)}; at_level 0 / above: {dict(placed)}; drops: {dict(drops)} by {dict(anchors)}")
    assert set(ops) == set(P2.X.OPS) and set(forms) == {"render", "tensor", "pair"}
    assert {"ball", "list", "empty"} <= set(trees) and placed[0] and placed[1]
    assert drops["nothing"] >= 2 and drops["some"] >= 2 and anchors["floor"] and anchors["box"]


def test_rests_before_the_new_writers_and_the_calls_that_write_nothing(sessions2, plans2, O):
    """worst_combinations(): a 34-frame rest of the owner directly before a combine through the owner, a combine through the
    sharing context and a drop that drops, each followed by a frame that must not be replayed; a 34-frame rest directly before
    a drop that drops nothing, a rects and a components, none of which forbids the replay of the frame behind it; and each of
    these three between two frames that must be replayed (the Tracker says `must` only for the first DEAL_LEARN frames of an
    accepted rest, so these stand in a shorter rest)"""
    assert not S.culls(P.Views(O).uniforms(P.REST_POSE), 2), "the resting pose is culled: the deal would never replay"
    seen, between = collections.Counter(), collections.Counter()
    for name, steps in sessions2.items():
        frames_of, k = [], 0
        for n in P.owner_ops(steps)[1]:
            frames_of.append(plans2[name][k:k + n])
            k += n
        assert k == len(plans2[name])

        def kind_of(s):
            if s["mutates"]:
                return s["op"].kind + (" through the sharing context" if s["via"] else "")
            return s["op"].kind + (" that writes nothing" if s["op"].kind == "drop" else "")

        for i, s in enumerate(steps[:-1]):
            nxt = steps[i + 1]
            after = next((f for f in frames_of[i + 1:] if f), None)
            if s["op"].kind != "frame" or nxt["op"].kind not in ("combine", "drop", "rects", "components") or after is None:
                continue
            first = after[0]["launches"][0]["replay"]
            if not nxt["mutates"]:
                assert nxt["writes"] == 0
                if frames_of[i][-1]["launches"][0]["replay"] == 1 and first == 1:
                    between[kind_of(nxt)] += 1
            if s["op"] != S.Op("frame", P.REST_POSE, 34):
                continue
            replay = [F["launches"][0]["replay"] for F in frames_of[i]]
            if nxt["mutates"]:
                assert replay.count(1) >= S.DEAL_LEARN // 2, f"{name}, op {i}: the rest replays {replay.count(1)} frames for certain"
                assert first == 0, f"{name}, op {i + 1}: a replay straight after a write"
            else:
                assert 0 not in replay and first != 0, f"{name}, op {i + 1}: a call that writes nothing ends the rest"
            seen[kind_of(nxt)] += 1
    print(f"a 34-frame rest directly before: {dict(seen)}; between two frames that must be replayed: {dict(between)}")
    for kind in ("combine", "combine through the sharing context", "drop that writes nothing", "rects", "components"):
        assert seen[kind], kind
    assert seen["drop"] + seen["drop through the sharing context"] >= 1
    for kind in ("drop that writes nothing", "rects", "components"):
        assert between[kind], kind
