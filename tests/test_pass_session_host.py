"""What makes the pass sessions (tests/test_pass_session_gpu.py) worth running, held on the host: the restatements agree with
each other on the composed inputs the GPU will see -- after every mutating op the model's words, sampled over the whole grid,
equal a dense grid that only the per-cell contracts update -- and the seeded sessions and worst_transitions() together put every
pass directly behind every mutating pass and behind every refusal of a pass it shares a workspace with, cross a scan tile and
drop back under it, feed the passes layouts no builder made, and rest long enough for the static deal before writes of every
kind.  Without these conditions the GPU test could pass while checking nothing.  The tallies are printed (-s shows them)."""
import collections

import numpy as np
import pytest

import pass_session_ops as P
import session_ops as S


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
